"""tests/bow_vector_ref.py, the numpy specification of ms_bow_vector, against a literal walk of DBoW2's batch transform as the
mirror's BowIndex::assembleVector states it: a Python dict filled in feature order (v[word] += weight for weight > 0), then normalised over
sorted(dict).  And the order-sensitive input the GPU test uses: three other ways of summing must give different bits, so that a kernel with
a reordered sum cannot pass."""
import numpy as np
import pytest

import bow_vector_ref as R

VOCAB = 5000


def literal(word, weight):
    v = {}
    for i in range(len(word)):
        if not (weight[i] > 0):
            continue
        k = int(word[i])
        v[k] = v.get(k, np.float64(0.0)) + np.float64(weight[i])      # std::map's operator[] starts a new entry at 0.0
    norm = np.float64(0.0)
    for k in sorted(v):
        norm = norm + np.abs(v[k])
    if norm > 0.0:
        for k in sorted(v):
            v[k] = v[k] / norm
    ks = sorted(v)
    return np.array(ks, np.int32).reshape(-1), np.array([v[k] for k in ks], np.float64).reshape(-1)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("name", list(R.cases(VOCAB)))
def test_the_restatement_is_the_literal_walk(name):
    word, weight = R.cases(VOCAB)[name]
    words, values, n_words, n_bad = R.bow_vector(word, weight, VOCAB)
    lw, lv = literal(word, weight)
    assert same_bits(words, lw) and same_bits(values, lv) and n_words == len(lw) and n_bad == 0
    assert (np.diff(words) > 0).all() and words.dtype == np.int32 and values.dtype == np.float64
    if n_words:
        assert abs(values.sum() - 1.0) < 1e-12 and (values > 0).all()


def test_the_named_cases_are_what_they_say():
    c = R.cases(VOCAB)
    assert R.bow_vector(*c["n = 0"], VOCAB)[2:] == (0, 0) and R.bow_vector(*c["all weights zero"], VOCAB)[2:] == (0, 0)
    assert R.bow_vector(*c["one word"], VOCAB)[2] == 1 and R.bow_vector(*c["all distinct"], VOCAB)[2] == 300
    assert (c["word -1 at weight 0"][0] == -1).sum() == 60 and R.bow_vector(*c["word -1 at weight 0"], VOCAB)[3] == 0
    w, wt = c["nan and negative weights"]
    kept = wt > 0
    assert np.isnan(wt).any() and (wt < 0).any() and same_bits(R.bow_vector(w, wt, VOCAB)[0], np.unique(w[kept]).astype(np.int32))
    assert R.bow_vector(*c["stop words"], VOCAB)[2] <= R.bow_vector(*c["duplicate words"], VOCAB)[2]


def test_n_bad_counts_words_outside_the_vocabulary_and_values_that_are_not_finite():
    word = np.array([3, 9, -1, 10, 4, 10], np.int32)
    weight = np.array([1.0, 2.0, 0.5, 0.25, 0.0, 1.0])
    assert R.bow_vector(word, weight, 11)[3] == 1 and R.bow_vector(word, weight, 10)[3] == 3      # -1; -1 and both keypoints on word 10
    weight[2] = 0.0
    assert R.bow_vector(word, weight, 11)[3] == 0 and R.bow_vector(word, weight, 10)[3] == 2
    word[4] = 77                                             # weight 0: never looked at
    assert R.bow_vector(word, weight, 11)[3] == 0
    weight[0] = np.inf                                       # inf / inf
    words, values, n_words, n_bad = R.bow_vector(word, weight, 11)
    assert n_bad == 1 and np.isnan(values[0]) and (values[1:] == 0).all()


def pairwise(terms):
    terms = [np.float64(t) for t in terms]
    if not terms:
        return np.float64(0.0)
    while len(terms) > 1:
        terms = [terms[i] + terms[i + 1] if i + 1 < len(terms) else terms[i] for i in range(0, len(terms), 2)]
    return terms[0]


def in_order(terms):
    s = np.float64(0.0)
    for t in terms:
        s = s + np.float64(t)
    return s


def summed(word, weight, segment, norm_of):
    """the vector with the segment sums and the norm taken by the given rules (functions of the terms in the specified order)"""
    kept = [i for i in range(len(word)) if weight[i] > 0]
    words = sorted({int(word[i]) for i in kept})
    values = [segment([weight[i] for i in kept if word[i] == w]) for w in words]
    norm = norm_of([np.abs(v) for v in values])
    return np.array([v / norm for v in values], np.float64)


def test_the_order_sensitive_input_separates_every_reordering():
    word, weight, vocab = R.order_sensitive()
    assert R.ORDER_SEED == 5 and len(word) == 600 and 2.0 ** -30 <= weight.min() < 2.0 ** -25 and 2.0 ** 5 < weight.max() <= 2.0 ** 10
    words, values, n_words, n_bad = R.bow_vector(word, weight, vocab)
    assert n_bad == 0 and n_words == 40 and same_bits(values, literal(word, weight)[1])
    assert same_bits(values, summed(word, weight, in_order, in_order))
    backwards = lambda terms: in_order(terms[::-1])
    others = {"segments in descending i": summed(word, weight, backwards, in_order), "the norm in descending word order": summed(word, weight, in_order, backwards),
              "pairwise segments": summed(word, weight, pairwise, in_order), "a pairwise norm": summed(word, weight, in_order, pairwise)}
    for name, v in others.items():
        assert not same_bits(values, v), name
        assert np.allclose(values, v, rtol=1e-12, atol=0), name              # the same vector up to rounding: only the order differs
