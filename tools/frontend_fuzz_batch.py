"""Differential fuzz of the front end in BATCHES against the CPU oracle: the sibling of tools/frontend_fuzz.py for what only a batch exercises -- k_fast's
raised threshold prunes only when a frame's tiles run at different times, i.e. with many frames per call.  N random configurations,
64 .. 160 frames per call (a few different frames, each at many places of the batch, so the oracle runs once per different frame), small quotas as well as
large ones, with and without a minimum distance; every frame's keypoints, angles and descriptors bit for bit, and the detector's candidate counts never above
the unpruned ones of a one-frame call.  usage: python tools/frontend_fuzz_batch.py [N] [seed] [px [map]]"""
import os, sys
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("slam-module_amd", "oracle"): sys.path.insert(0, os.path.join(R, p))
import numpy as np, mi355slam, mso
N = int(sys.argv[1]) if len(sys.argv) > 1 else 40
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 11)
ctx = mi355slam.Context(0)
done = bad = pruned_cfgs = 0
while done < N:
    w = int(rng.choice([248, 496, 744, 256, 512])) + int(rng.integers(-9, 10)) if rng.random() < 0.5 else int(rng.integers(120, 800))
    h = int(rng.integers(60, 420))
    levels = int(rng.integers(1, 6)); sf = float(rng.choice([1.1, 1.2, 1.25, 1.5, 2.0]))
    if min(w, h) / sf ** (levels - 1) < 41: continue
    thr = int(rng.integers(4, 50)); kp = int(rng.choice([20, 60, 150, 400, 1500])); kind = int(rng.integers(0, 3))
    md = float(rng.choice([0.0, 0.0, 8.0, 25.0]))
    n_frames = int(rng.integers(64, 161)); distinct = int(rng.integers(1, 5))
    imgs = []
    for d in range(distinct):
        if kind == 0: img = rng.integers(0, 256, (h, w), dtype=np.uint8)
        elif kind == 1: img = mso.synth_frame(w, h, int(rng.integers(0, 1000)))
        else: img = (rng.integers(0, 4, (h // 8 + 1, w // 8 + 1), dtype=np.uint8) * 80).repeat(8, 0).repeat(8, 1)[:h, :w].copy()
        imgs.append(np.ascontiguousarray(img))
    which = rng.integers(0, distinct, n_frames)
    batch = np.ascontiguousarray(np.stack(imgs)[which])
    ocfg = mso.cfg(levels=levels, scale_factor=sf, max_kpts=kp, fast_threshold=thr, min_distance=md)
    want = [mso.orb_extract(ocfg, img) for img in imgs]
    ex = mi355slam.OrbExtractor(ctx, w, h, levels=levels, scale_factor=sf, max_kpts=kp, fast_threshold=thr, max_batch=n_frames + int(rng.integers(0, 3)), min_distance=md)
    if len(sys.argv) > 3: ex.set_resize_plan(int(sys.argv[3]), int(sys.argv[4]) if len(sys.argv) > 4 else 0)      # [px [map]]: force the resize kernel / its grid mapping
    full = []
    for img in imgs:                                 # a one-frame call prunes nothing: its counts are the unpruned ones
        ex.extract(img[None]); full.append(ex.last_candidate_counts()[0])
    if rng.random() < 0.5:
        ex.extract(batch)                            # host frames (four pieces)
    else:
        dev = ctx.upload(batch); ex.extract(dev, n_frames=n_frames, frame_stride=w * h, row_stride=w); ctx.sync(); dev.free()
    counts = ex.last_candidate_counts()
    ok = bool((counts <= np.stack(full)[which]).all())
    pruned_cfgs += int(counts.sum() < np.stack(full)[which].sum())
    for f in range(n_frames):
        got, wnt = ex.download(f), want[which[f]]
        ok = ok and len(got["x"]) == len(wnt["x"]) and all(np.array_equal(got[k].view(np.uint32), wnt[k].view(np.uint32)) for k in ("x", "y", "angle")) \
            and np.array_equal(got["octave"], wnt["octave"]) and np.array_equal(got["desc"], wnt["desc"])
    done += 1
    if not ok:
        bad += 1
        print("MISMATCH", dict(w=w, h=h, levels=levels, sf=sf, thr=thr, kp=kp, kind=kind, md=md, n_frames=n_frames, distinct=distinct), flush=True)
    ex.close()
print("batch fuzz: %d configurations (%d of them pruned something), %d mismatches" % (done, pruned_cfgs, bad))
sys.exit(1 if bad else 0)
