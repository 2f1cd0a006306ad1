"""The specification of ms_bow_vector and ms_bow_db_add_words in numpy: DBoW2's BowVector::addWeight sums and normalize(L1)
as the mirror's BowIndex::assembleVector pins them, with the order of every addition written out.

  keep       keypoint i is kept iff weight[i] > 0 as written (a NaN, a zero, a negative weight, a stop word are skipped; their word is
             never looked at)
  order      the kept keypoints by (word, i)
  entries    one per distinct word, ascending
  value      0.0, then the kept weights of the word one by one in ascending i, float64
  norm       0.0, then fabs(value) entry by entry in ascending word order
  normalise  iff norm > 0.0 every value becomes value / norm
  n_bad      kept keypoints with a word outside [0, vocab_words), plus the final values that are not finite

numpy's float64 scalars add and divide as IEEE doubles, one rounding per operation and nothing fused, so the loops below are the rule."""
import numpy as np


def bow_vector(word, weight, vocab_words):
    """Returns (words int32 strictly ascending, values float64, n_words, n_bad)."""
    word = np.asarray(word, np.int32).reshape(-1)
    weight = np.asarray(weight, np.float64).reshape(-1)
    assert len(word) == len(weight)
    kept = [i for i in range(len(weight)) if weight[i] > 0]
    n_bad = sum(1 for i in kept if not 0 <= int(word[i]) < vocab_words)
    kept.sort(key=lambda i: (int(word[i]), i))
    words, values = [], []
    for i in kept:
        if not words or words[-1] != int(word[i]):
            words.append(int(word[i]))
            values.append(np.float64(0.0))
        values[-1] = values[-1] + weight[i]
    norm = np.float64(0.0)
    for v in values:
        norm = norm + np.abs(v)
    with np.errstate(invalid="ignore", over="ignore"):
        if norm > 0.0:
            values = [v / norm for v in values]
    values = np.array(values, np.float64).reshape(-1)
    n_bad += int((~np.isfinite(values)).sum())
    return np.array(words, np.int32).reshape(-1), values, len(words), n_bad


ORDER_SEED = 5               # separates all three reorderings (asserted by tests/test_bow_vector_ref.py); pick another and record it here if it ever does not


def order_sensitive(seed=ORDER_SEED, n=600, n_distinct=40, vocab_words=1000):
    """The input no reordered sum passes: weights 2^-30 .. 2^10 (log-uniform) over n_distinct words, about n / n_distinct keypoints each, in a
    shuffled order.  tests/test_bow_vector_ref.py asserts that summing a segment in descending i, the norm in descending word order, and a
    pairwise sum of either each give different bits from the specified order for this seed."""
    rng = np.random.default_rng(seed)
    words = np.sort(rng.choice(vocab_words, n_distinct, replace=False)).astype(np.int32)
    word = words[rng.integers(0, n_distinct, n)].astype(np.int32)
    weight = np.exp2(rng.uniform(-30.0, 10.0, n))
    return word, weight, vocab_words


def cases(vocab_words=5000):
    """Named inputs (word, weight) that the CPU and the GPU tests share."""
    rng = np.random.default_rng(17)
    out = {}
    w = rng.integers(0, 50, 300).astype(np.int32)
    out["duplicate words"] = (w, rng.random(300) * 3 + 0.01)
    wt = rng.random(300) * 3 + 0.01
    wt[rng.random(300) < 0.3] = 0.0
    out["stop words"] = (w, wt)
    wt = rng.random(300) * 3 + 0.01
    wt[::7] = np.nan
    wt[3::11] = -1.5
    wt[5::13] = -np.inf
    out["nan and negative weights"] = (w, wt)
    w2, wt = w.copy(), rng.random(300) + 0.5
    w2[::5] = -1
    wt[::5] = 0.0
    out["word -1 at weight 0"] = (w2, wt)
    out["n = 0"] = (np.zeros(0, np.int32), np.zeros(0))
    out["all weights zero"] = (w, np.zeros(300))
    out["one word"] = (np.full(300, 77, np.int32), rng.random(300) + 0.1)
    out["all distinct"] = (rng.permutation(vocab_words)[:300].astype(np.int32), rng.random(300) + 0.1)
    return out
