"""Times ms_keyframe_admit, the arrival of a keyframe on the device map tables, against the path it replaces.

  shape   2 000 keypoints (64 of them tracker features) in a device keypoint view of the extractor's layout, a vocabulary of k = 10, L = 6
          (1 111 111 nodes), tables of 8 slots x 2 048, a 640 x 480 depth image.
  device  ms_keyframe_admit: one synchronous call through the Python binding, every host output wanted.
  before  what an application did without it, with every device buffer allocated beforehand: the seven downloads of ms_orb_download; the
          upload of the descriptors, ms_bow_transform and its three downloads; on the host the depths, the bearings, ms_feature_search_sort and
          the node lists (numpy: a stable argsort, where the mirror fills a std::map); then the uploads -- eleven arrays of the keyframe, four
          rows of the keypoint table, the pool slice, the kf_mp row and the pose.

Host clock around the synchronous calls, three warm-ups, the best and the mean of --reps calls, the slot's row restored outside the timed
span.  The tables, the frame arrays and the host outputs of both paths are compared for equal bits.  Prints one JSON line.
python tools/keyframe_admit_probe.py [--reps 20] [--n 2000]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "slam-module_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import keyframe_admit_ref as R        # noqa: E402
import mi355slam                      # noqa: E402

CAM = dict(fx=520.25, fy=519.5, cx=318.75, cy=241.125)
CAM6 = (CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"], 640, 480)
N_KF, STRIDE, SLOT = 8, 2048, 5


def make_vocab(k, depth, seed=3):
    """A full k-ary tree numbered breadth first, as DBoW2 numbers it; a child's descriptor is its parent's with about a quarter of the bits flipped."""
    rng = np.random.default_rng(seed)
    words = lambda n: rng.integers(0, 2 ** 32, (n, 8), dtype=np.uint64).astype(np.uint32)
    parent, desc, first = [np.zeros(1, np.int32)], [np.zeros((1, 8), np.uint32)], 0
    level = np.zeros((1, 8), np.uint32)
    for lv in range(1, depth + 1):
        n = len(level) * k
        level = words(n) if lv == 1 else np.repeat(level, k, axis=0) ^ (words(n) & words(n))
        parent.append(np.repeat(np.arange(first, first + n // k, dtype=np.int32), k))
        desc.append(level)
        first += n // k
    parent, desc = np.concatenate(parent), np.concatenate(desc)
    n, leaves = len(parent), len(level)
    word, weight = np.full(n, -1, np.int32), np.zeros(n)
    word[n - leaves:] = np.arange(leaves, dtype=np.int32)
    weight[n - leaves:] = np.where(rng.random(leaves) < 0.05, 0.0, rng.random(leaves) * 9 + 0.01)
    return dict(parent=parent, desc=desc, weight=weight, word=word, depth_levels=depth)


def clock(fn, reps, before):
    best, total, out = float("inf"), 0.0, None
    for i in range(3 + reps):
        before()
        t0 = time.perf_counter()
        out = fn()
        dt = time.perf_counter() - t0
        if i >= 3:
            best, total = min(best, dt), total + dt
    return dict(best_ms=round(best * 1e3, 4), mean_ms=round(total / reps * 1e3, 4)), out


def put(ctx, buf, arr, offset=0):
    arr = np.ascontiguousarray(arr)
    ctx.check(mi355slam.lib().ms_dev_upload(ctx._h, C.c_void_p(buf.ptr + offset), mi355slam._vp(arr), C.c_size_t(arr.nbytes)), "ms_dev_upload")


def probe(ctx, n, reps):
    arrays = make_vocab(10, 6)
    vocab = mi355slam.BowVocabulary(ctx, arrays["parent"], arrays["desc"], arrays["weight"], arrays["word"], 6)
    frame = R.synth_frame(n, 5, n_tracked=64)
    leaves = np.flatnonzero(arrays["word"] >= 0)
    rng = np.random.default_rng(6)
    frame["desc"] = arrays["desc"][rng.choice(leaves, n)] ^ (rng.integers(0, 2 ** 32, (n, 8), dtype=np.uint64).astype(np.uint32) & rng.integers(0, 2 ** 32, (n, 8), dtype=np.uint64).astype(np.uint32)
                                                              & rng.integers(0, 2 ** 32, (n, 8), dtype=np.uint64).astype(np.uint32))
    ids, track_depth = np.arange(100, 164, dtype=np.int32), np.where(rng.random(64) < 0.5, rng.random(64) * 5, -1).astype(np.float32)
    image = (rng.random((480, 640)) * 20).astype(np.float32)
    d_image = ctx.upload(image)
    cap = n + 64
    # the view, one frame
    vb = dict(count=ctx.upload(np.array([n], np.int32)))
    for k, dt, w in (("x", np.float32, 1), ("y", np.float32, 1), ("angle", np.float32, 1), ("octave", np.int32, 1), ("desc", np.uint32, 8), ("track_id", np.int32, 1)):
        a = np.zeros((cap, w), dt)
        a[:n] = np.asarray(frame[k], dt).reshape(n, w)
        vb[k] = ctx.upload(a)
    view = mi355slam.keypoints_view(cap, vb["count"], vb["x"], vb["y"], vb["angle"], vb["octave"], vb["desc"], vb["track_id"])
    t = R.empty_tables(N_KF, STRIDE, N_KF * STRIDE, 1)
    base = SLOT * STRIDE
    pose = np.arange(12, dtype=np.float64)
    sets = [{k: ctx.upload(t[k]) for k in R.TABLES} for _ in range(2)]      # 0: the device path's tables, 1: the host path's
    frames = [mi355slam.AdmitFrame(ctx, STRIDE) for _ in range(2)]
    d_desc, d_word, d_weight, d_node = ctx.alloc(32 * cap), ctx.alloc(4 * cap), ctx.alloc(8 * cap), ctx.alloc(4 * cap)
    args = dict(slot=SLOT, desc_base=base, pose=pose, cam=CAM6, levels_up=4, vocab=vocab, track_ids=ids, track_depth=track_depth, depth_image=d_image, depth_width=640,
                depth_height=480)

    def device():
        rc, res = mi355slam.keyframe_admit_device(ctx, view, 0, sets[0], N_KF, STRIDE, 50, N_KF * STRIDE, args, frames[0])
        ctx.check(rc, "ms_keyframe_admit")
        return res

    def host():
        cnt = int(vb["count"].download(np.int32, (1,))[0])                  # ms_orb_download: the count, then six arrays
        kp = {k: vb[k].download(dt, (cnt, w) if w > 1 else (cnt,)) for k, dt, w in (("x", np.float32, 1), ("y", np.float32, 1), ("angle", np.float32, 1), ("octave", np.int32, 1),
                                                                                     ("desc", np.uint32, 8), ("track_id", np.int32, 1))}
        put(ctx, d_desc, kp["desc"])                                         # BowIndex::transform
        ctx.check(mi355slam.lib().ms_bow_transform(ctx._h, vocab._h, mi355slam._vp(d_desc), cnt, 4, mi355slam._vp(d_word), mi355slam._vp(d_weight), mi355slam._vp(d_node)),
                  "ms_bow_transform")
        ctx.sync()
        word, weight, node = d_word.download(np.int32, (cnt,)), d_weight.download(np.float64, (cnt,)), d_node.download(np.int32, (cnt,))
        at = R.track_indices(kp["track_id"], ids)                           # processKeyPoints
        depth = R.depths(kp["x"], kp["y"], at, track_depth, image)
        bearing = R.bearing(CAM, kp["x"], kp["y"])
        sx, sy, si = mi355slam.feature_search_sort(kp["x"], kp["y"])        # FeatureSearch::create
        node_id, node_start, kp_idx = R.node_lists(dict(kp, word=word, weight=weight, node=node))
        b = frames[1].bufs                                                  # DeviceKeyframe's constructor: eleven arrays
        for name, a in (("desc", kp["desc"]), ("angle", kp["angle"]), ("octave", kp["octave"]), ("bearing", bearing), ("usable", np.ones(cnt, np.uint8)), ("sorted_x", sx),
                        ("sorted_y", sy), ("sorted_idx", si), ("node_id", node_id), ("node_start", node_start), ("kp_idx", kp_idx)):
            put(ctx, b[name], a)
        T = sets[1]
        row = 4 * SLOT * STRIDE                                             # DeviceKeypointTable::update, the pool, the row, the pose
        put(ctx, T["kp_x"], kp["x"], row); put(ctx, T["kp_y"], kp["y"], row); put(ctx, T["kp_octave"], kp["octave"], row); put(ctx, T["kp_depth"], depth, row)
        put(ctx, T["desc_pool"], kp["desc"], 32 * base)
        put(ctx, T["kf_mp"], np.full(STRIDE, -1, np.int32), row)
        put(ctx, T["kf_pose"], pose, 96 * SLOT)
        ctx.sync()
        return dict(counts=np.array([cnt, len(node_id), len(kp_idx)], np.int32), kp_track=kp["track_id"], word=word, weight=weight, sorted_x=sx, sorted_y=sy, sorted_idx=si,
                    octave=kp["octave"], desc=kp["desc"])

    try:
        out = dict(n=n, n_tracks=64, vocabulary_nodes=int(len(arrays["parent"])), stride=STRIDE)
        out["admit"], got = clock(device, reps, lambda: None)
        out["host_path"], old = clock(host, reps, lambda: None)
        same = lambda a, b: a.dtype == b.dtype and a.tobytes() == b.tobytes()
        equal = all(same(np.ascontiguousarray(got[k]).reshape(-1), np.ascontiguousarray(old[k]).reshape(-1)) for k in old)
        equal = equal and all(same(sets[0][k].download(t[k].dtype, t[k].shape), sets[1][k].download(t[k].dtype, t[k].shape)) for k in R.TABLES)
        f0, f1 = frames[0].download(), frames[1].download()
        cnt, n_nodes, listed = (int(v) for v in got["counts"])
        for k in R.FRAME:
            m = n_nodes + 1 if k == "node_start" else n_nodes if k == "node_id" else listed if k == "kp_idx" else cnt
            equal = equal and same(f0[k][:m], f1[k][:m])
        out.update(n_nodes=n_nodes, listed=listed, equal_bits=bool(equal))
        return out
    finally:
        for b in list(vb.values()) + [d_image, d_desc, d_word, d_weight, d_node] + [x for s in sets for x in s.values()]:
            b.free()
        for f in frames:
            f.free()
        vocab.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--n", type=int, default=2000)
    a = ap.parse_args()
    ctx = mi355slam.Context(0)
    try:
        print(json.dumps(dict(probe="keyframe_admit", reps=a.reps, result=probe(ctx, a.n, a.reps))))
    finally:
        ctx.close()


if __name__ == "__main__":
    main()
