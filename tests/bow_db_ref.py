"""Plain-Python restatement of the reference's keyframe database (BowIndex::add / remove / getBowSimilar) and a generator of
synthetic databases for the ms_bow_db tests.

The restatement keeps what the reference keeps: one posting list per word, filled by add and emptied of an id by remove.  A query
counts shared words per id into a dict, takes the largest count, keeps the ids whose count exceeds the truncated float32 threshold,
scores each with DBoW2's L1 score (summed in ascending word order with Python floats, which are IEEE doubles), orders them by score
descending with ties in (map_id, kf_id) order (a stable sort of the ids in std::map order) and cuts below best * score_ratio in float32.
"""
import numpy as np

CURRENT_MAP_ID = 1000


def l1_score(qw, qv, ew, ev):
    """DBoW2 L1Scoring::score(query, entry) as a float32: -sum(|v - w| - |v| - |w|) / 2 over the common words, ascending."""
    vals = dict(zip((int(x) for x in ew), (float(x) for x in ev)))
    s = 0.0
    for w, v in zip(qw, qv):
        w = int(w)
        if w in vals:
            wi, vi = vals[w], float(v)
            s += abs(vi - wi) - abs(vi) - abs(wi)
    return np.float32(-s / 2.0)


class RefIndex:
    """The inverted index: word -> list of (map_id, kf_id), plus every entry's vector (what the reference reads through MapDB)."""

    def __init__(self):
        self.lists = {}
        self.vec = {}

    def add(self, map_id, kf_id, words, values):
        key = (int(map_id), int(kf_id))
        assert key not in self.vec
        self.vec[key] = (np.asarray(words, np.int32).copy(), np.asarray(values, np.float64).copy())
        for w in self.vec[key][0]:
            self.lists.setdefault(int(w), []).append(key)

    def remove(self, map_id, kf_id):
        key = (int(map_id), int(kf_id))
        if key not in self.vec: return                  # the reference's loop finds nothing to erase
        for w in self.vec.pop(key)[0]:                  # the id can only be in the lists of its own words
            self.lists[int(w)].remove(key)

    def __len__(self):
        return len(self.vec)

    def query(self, words, values, exclude=None, min_in_common_ratio=0.8, score_ratio=0.75):
        """Returns (map_ids i32, kf_ids i32, scores f32) in the reference's order."""
        shared = {}                                      # id -> [(word, query value)] in ascending word order; its length is the count
        ex = None if exclude is None else (int(exclude[0]), int(exclude[1]))
        for w, v in zip(words, values):
            for key in self.lists.get(int(w), ()):
                if key == ex: continue
                shared.setdefault(key, []).append((int(w), float(v)))
        empty = (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32))
        if not shared: return empty
        max_in_common = max(len(c) for c in shared.values())
        min_in_common = int(np.float32(min_in_common_ratio) * np.float32(max_in_common))      # float32 product, truncated
        similar = []
        for key in sorted(shared):                                                           # std::map order
            if len(shared[key]) > min_in_common:
                ew, ev = self.vec[key]
                pos = np.searchsorted(ew, [w for w, _ in shared[key]])
                s = 0.0
                for (w, vi), p in zip(shared[key], pos):                                     # L1Scoring::score, ascending words
                    wi = float(ev[p])
                    s += abs(vi - wi) - abs(vi) - abs(wi)
                similar.append((key, np.float32(-s / 2.0)))
        if not similar: return empty
        similar.sort(key=lambda p: -float(p[1]))                                             # stable: ties keep id order
        min_score = np.float32(similar[0][1] * np.float32(score_ratio))
        cut = len(similar)
        for i, (_, s) in enumerate(similar):
            if s < min_score:
                cut = i
                break
        similar = similar[:cut]
        return (np.array([k[0] for k, _ in similar], np.int32), np.array([k[1] for k, _ in similar], np.int32),
                np.array([s for _, s in similar], np.float32))

    def query_id(self, map_id, kf_id, **kw):
        w, v = self.vec[(int(map_id), int(kf_id))]
        return self.query(w, v, exclude=(map_id, kf_id), **kw)


def normalize_l1(values):
    v = np.asarray(values, np.float64)
    n = 0.0
    for x in v: n += abs(float(x))                                                          # BowVector::normalize(L1), in word order
    return v / n if n > 0 else v


class Synth:
    """Keyframes that revisit a few "places": each place has a word set drawn with Zipf-like frequencies, a visit keeps most of it,
    drops some words, adds others and perturbs the weights.  Vectors are sorted by word and L1-normalised."""

    def __init__(self, seed, n_words=1_000_000, n_places=20, words_per_place=(300, 1000), zipf=1.1):
        self.rng = np.random.default_rng(seed)
        self.n_words = n_words
        lo, hi = words_per_place
        self.places = []
        for _ in range(n_places):
            k = int(self.rng.integers(lo, hi + 1))
            self.places.append(self._draw(k, zipf))

    def _draw(self, k, zipf):
        ranks = np.minimum(self.rng.zipf(zipf, 4 * k), self.n_words)          # a frequent head, a long tail
        w = np.unique(np.minimum(ranks * 7919 + self.rng.integers(0, 7919, len(ranks)), self.n_words - 1))
        if len(w) > k: w = np.sort(self.rng.choice(w, k, replace=False))
        return w.astype(np.int32)

    def keyframe(self, place=None, keep=0.8, extra=50):
        if place is None: place = int(self.rng.integers(0, len(self.places)))
        base = self.places[place]
        kept = base[self.rng.random(len(base)) < keep]
        add = self.rng.integers(0, self.n_words, extra)
        w = np.unique(np.concatenate([kept, add])).astype(np.int32)
        v = normalize_l1(self.rng.random(len(w)) * 2.0 + 0.01)
        return w, v


def make_db(seed, n, n_maps=3, **kw):
    """n entries over n_maps map ids that share kf ids (map CURRENT_MAP_ID and 0 .. n_maps - 2): [(map_id, kf_id, words, values)]."""
    s = Synth(seed, **kw)
    maps = [CURRENT_MAP_ID] + list(range(n_maps - 1))
    out = []
    for i in range(n):
        w, v = s.keyframe()
        out.append((maps[i % n_maps], i // n_maps, w, v))
    return s, out
