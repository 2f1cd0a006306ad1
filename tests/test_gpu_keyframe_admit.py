"""ms_keyframe_admit on the device against tests/keyframe_admit_ref.py, its specification: every table, every frame array and
every host output bit for bit, canaries behind every buffer, the same bytes on a second run.  The real extractor's view against today's path
(ms_orb_download, the host sort, ms_bow_transform and the host's node lists), with the matchers, the radius search and ms_match_tracked run on
admitted and on host-built keyframes; synthetic views at the sizes where a path changes (0, 1, one more than a workgroup, the full row, ties in
y across a workgroup boundary, one node, 600 nodes, stop words, every source of a depth); every refusal with all bytes untouched; no allocation
after warm-up; `usable` against ms_unbound_mask."""
import ctypes as C
import functools

import numpy as np
import pytest

import bow_synth
import keyframe_admit_ref as R
import mi355slam

pytestmark = pytest.mark.gpu
CAN, PAD = 0x5A, 16
CAM = dict(fx=520.25, fy=519.5, cx=318.75, cy=241.125)
CAM6 = (CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"], 640, 480)
POSE = np.arange(12, dtype=np.float64) * 0.25 - 1.0
HOST = tuple(k for k, _, _ in mi355slam._ADMIT_HOST)
HOST_REF = dict(kp_track="kp_track", word="word", weight="weight", sorted_x="h_sorted_x", sorted_y="h_sorted_y", sorted_idx="h_sorted_idx", octave="h_octave", desc="h_desc")
VIEW = (("x", np.float32, 1), ("y", np.float32, 1), ("angle", np.float32, 1), ("octave", np.int32, 1), ("desc", np.uint32, 8), ("track_id", np.int32, 1))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.size == b.size and a.tobytes() == b.tobytes()


def canary(nbytes):
    return np.full(nbytes, CAN, np.uint8)


def with_canary(a):
    return np.concatenate([np.ascontiguousarray(a).reshape(-1).view(np.uint8), canary(PAD)])


@functools.lru_cache(maxsize=None)
def vocab_arrays(kind):
    if kind == "ragged":                                     # small, ragged, a third of the words are stop words
        return bow_synth.make_vocab(21, k=5, depth=3, ragged=0.3, stop_words=0.3)
    return bow_synth.make_vocab(22, k=10, depth=3, stop_words=0.1)      # 1000 leaves


def device_vocab(ctx, kind):
    v = vocab_arrays(kind)
    return mi355slam.BowVocabulary(ctx, v["parent"], v["desc"], v["weight"], v["word"], v["depth_levels"])


class Dev:
    """Tables, frame arrays and a two-frame view on the device, each with a canary behind it.  The view's frame 1 holds the keypoints; frame 0
    holds a decoy of another length, so that an entry point that forgets the frame offset is found out."""

    def __init__(self, ctx, tables, cap_kp, frame, capacity=None, fill=0xA5):
        self.ctx, self.t, self.cap = ctx, tables, cap_kp
        self.n_kf, self.stride = tables["kf_mp"].shape
        self.n_pool = len(tables["desc_pool"])
        self.tab = {k: ctx.upload(with_canary(tables[k])) for k in R.TABLES}
        self.before = R.frame_arrays(cap_kp, fill)
        self.out = {k: ctx.upload(with_canary(self.before[k])) for k in R.FRAME}
        self.struct = mi355slam.AdmitFrameC(cap_kp, *[self.out[k].ptr for k, _, _ in mi355slam._ADMIT_FRAME])
        self.set_view(frame, capacity)

    def set_view(self, frame, capacity=None):
        n = len(frame["x"])
        self.capacity = cap = capacity if capacity is not None else n + 5
        decoy = R.synth_frame(min(3, cap), 99)
        self.vbufs = {"count": self.ctx.upload(np.array([len(decoy["x"]), n], np.int32))}
        for k, dt, w in VIEW:
            a = np.zeros((2, cap, w), dt)
            a.view(np.uint8)[...] = 0x33                     # recognisable filler behind the count
            m = min(n, cap)
            a[0, :len(decoy["x"])] = np.asarray(decoy[k], dt).reshape(-1, w)
            a[1, :m] = np.asarray(frame[k], dt).reshape(-1, w)[:m]
            self.vbufs[k] = self.ctx.upload(with_canary(a))
        v = self.vbufs
        self.view = mi355slam.keypoints_view(cap, v["count"], v["x"], v["y"], v["angle"], v["octave"], v["desc"], v["track_id"])

    def call(self, args, host=HOST, view_frame=1, cap_kp=None, n_pool=None, n_mp=50):
        """The C call with a canary behind every host output.  Returns (rc, counts, host outputs cut to n)."""
        A, keep = mi355slam._admit_args(args)
        cap = self.cap
        arrs = {k: np.full((cap + PAD) * w, CAN, np.uint8).repeat(np.dtype(dt).itemsize).view(dt) for k, dt, w in mi355slam._ADMIT_HOST if k in host}
        H = mi355slam.AdmitHostC(*[arrs[k].ctypes.data if k in arrs else None for k in HOST])
        counts = np.full(3 + PAD, -77, np.int32)
        st = mi355slam.AdmitFrameC.from_buffer_copy(self.struct)
        st.cap_kp = cap if cap_kp is None else cap_kp
        vp = mi355slam._vp
        rc = mi355slam.lib().ms_keyframe_admit(self.ctx._h, C.byref(self.view), view_frame, vp(self.tab["kf_mp"]), self.n_kf, self.stride, n_mp, vp(self.tab["kp_x"]),
                                               vp(self.tab["kp_y"]), vp(self.tab["kp_octave"]), vp(self.tab["kp_depth"]), vp(self.tab["desc_pool"]),
                                               self.n_pool if n_pool is None else n_pool, vp(self.tab["kf_pose"]), C.byref(A), C.byref(st), C.byref(H), vp(counts))
        assert (counts[3:] == -77).all()
        n = int(counts[0]) if rc == 0 else 0
        got = {}
        for k, dt, w in mi355slam._ADMIT_HOST:
            if k in arrs:
                assert (arrs[k].view(np.uint8)[n * w * np.dtype(dt).itemsize:] == CAN).all(), k      # nothing behind n is written, nothing at all on a refusal
                got[k] = arrs[k][:n * w].copy()
        return rc, counts[:3].copy(), got

    def state(self):
        """Every table and frame array, their canaries and the view's bytes checked."""
        out = {}
        for name, bufs, like in (("tables", self.tab, self.t), ("frame", self.out, self.before)):
            for k, b in bufs.items():
                raw = b.download(np.uint8, (like[k].nbytes + PAD,))
                assert (raw[like[k].nbytes:] == CAN).all(), (name, k)
                out[k] = raw[:like[k].nbytes].view(like[k].dtype).reshape(like[k].shape)
        return out

    def free(self):
        for b in list(self.tab.values()) + list(self.out.values()) + list(self.vbufs.values()):
            b.free()


def descend(ctx, vocab, frame, levels_up):
    """today's path: ms_bow_transform on uploaded descriptors"""
    if len(frame["x"]) == 0:
        return dict(frame, word=np.zeros(0, np.int32), weight=np.zeros(0), node=np.zeros(0, np.int32))
    word, weight, node = vocab.transform(frame["desc"], levels_up)
    return dict(frame, word=word, weight=weight, node=node)


def check(dev, rc, counts, got, want, label=""):
    assert rc == want["rc"], (label, rc, want["rc"], mi355slam.lib().ms_last_error(dev.ctx._h))
    assert counts.tolist() == want["counts"].tolist(), (label, counts, want["counts"])
    state = dev.state()
    for k in R.TABLES + R.FRAME:
        assert same_bits(state[k], want[k]), (label, k)
    if rc == 0:
        for k in got:
            assert same_bits(got[k], want[HOST_REF[k]]), (label, k)
    return state


def admit_and_check(ctx, frame, tables, cap_kp, args, vocab=None, label="", capacity=None, n_mp=50, twice=True):
    """One call on fresh buffers against the restatement, and a second one on fresh buffers that must give the same bytes."""
    with_words = descend(ctx, vocab, frame, args.get("levels_up", 4)) if vocab is not None else frame
    want = R.admit(tables, n_mp, with_words, args["slot"], args["desc_base"], args["pose"], CAM, cap_kp, view_capacity=capacity, track_ids=args.get("track_ids"),
                   track_depth=args.get("track_depth"), depth_image=args.get("image"), before=R.frame_arrays(cap_kp, 0xA5))
    args = dict(args, vocab=vocab, cam=CAM6)
    image = None
    if args.get("image") is not None:
        image = ctx.upload(args["image"])
        args.update(depth_image=image, depth_height=args["image"].shape[0], depth_width=args["image"].shape[1])
    runs = []
    for _ in range(2 if twice else 1):
        dev = Dev(ctx, tables, cap_kp, frame, capacity)
        try:
            rc, counts, got = dev.call(args, n_mp=n_mp)
            runs.append((rc, counts, got, check(dev, rc, counts, got, want, label)))
        finally:
            dev.free()
    if image is not None:
        image.free()
    if twice:
        assert runs[0][0] == runs[1][0] and all(same_bits(runs[0][2][k], runs[1][2][k]) for k in runs[0][2]) and all(same_bits(runs[0][3][k], runs[1][3][k]) for k in runs[0][3])
    return want, runs[0]


# ---- 1. the real extractor
@pytest.fixture(scope="module")
def extracted(ctx, oracle):
    """Two shifted 640 x 480 frames with tracker features through ms_orb_extract; the view stays on the device."""
    imgs = np.stack([oracle.synth_frame(640, 480, 1000, 2 * i, i) for i in range(2)])
    ex = mi355slam.OrbExtractor(ctx, 640, 480, max_kpts=1000, max_tracks=64, max_batch=2)
    rng = np.random.default_rng(8)
    xy = [np.stack([rng.random(40) * 500 + 70, rng.random(40) * 340 + 70], 1).astype(np.float32) for _ in range(2)]
    ids = [np.arange(300, 340, dtype=np.int32), np.arange(320, 360, dtype=np.int32)]
    ex.extract(imgs, track_xy=xy, track_id=ids)
    ctx.sync()
    kps = [ex.download(f) for f in range(2)]
    yield ex, kps, ids
    ex.close()


def host_built(ctx, k, words):
    """a keyframe's matcher inputs the way they are built today: the host's node lists, everything uploaded"""
    ids, start, order = R.node_lists(words)
    n = len(k["x"])
    return mi355slam.FrameOnDevice(ctx, k["desc"], k["angle"], np.ones(n, np.uint8), None, octave=k["octave"], bearing=R.bearing(CAM, k["x"], k["y"]),
                                   csr=(ids if len(ids) else np.zeros(1, np.int32), start, order if len(order) else np.zeros(1, np.int32)))


def test_the_extractors_view_against_todays_path_and_the_consumers_agree(ctx, extracted):
    ex, kps, track_ids = extracted
    vocab = device_vocab(ctx, "ragged")
    view, cap, stride = ex.device_view(), ex.capacity, ex.capacity + 7
    n = [len(k["x"]) for k in kps]
    assert min(n) > 500 and all((k["track_id"] >= 0).sum() > 20 for k in kps)
    tables = R.empty_tables(3, stride, 2 * stride + 11, 1)
    rng = np.random.default_rng(2)
    image = (rng.random((480, 640)) * 20).astype(np.float32)
    d_image = ctx.upload(image)
    dev = Dev(ctx, tables, cap, kps[0])
    frames = [mi355slam.AdmitFrame(ctx, cap) for _ in range(2)]
    base = [5, 5 + n[0]]
    want, words, res = dict(tables), [], []
    try:
        for f in range(2):
            depth = np.where(rng.random(len(track_ids[f])) < 0.5, rng.random(len(track_ids[f])) * 5, -1).astype(np.float32)
            words.append(descend(ctx, vocab, kps[f], 1))
            want = R.admit({k: want[k] for k in R.TABLES}, 50, words[f], f, base[f], POSE + f, CAM, cap, track_ids=track_ids[f], track_depth=depth, depth_image=image)
            args = dict(slot=f, desc_base=base[f], pose=POSE + f, cam=CAM6, levels_up=1, vocab=vocab, track_ids=track_ids[f], track_depth=depth, depth_image=d_image,
                        depth_width=640, depth_height=480)
            rc, r = mi355slam.keyframe_admit_device(ctx, view, f, dev.tab, 3, stride, 50, dev.n_pool, args, frames[f])
            assert rc == 0, mi355slam.lib().ms_last_error(ctx._h)
            res.append(r)
            assert r["counts"].tolist() == want["counts"].tolist() and r["counts"][0] == n[f] and r["counts"][1] > 10
            got = frames[f].download()
            for k in R.FRAME:
                m = n[f] if k not in ("node_id", "node_start", "kp_idx") else want["counts"][1] + (k == "node_start") if k != "kp_idx" else want["counts"][2]
                assert same_bits(got[k][:m], want[k][:m]), (f, k)
            for k in HOST:
                assert same_bits(r[k], want[HOST_REF[k]]), (f, k)
            # today's path: the download, the library's host sort, the host's BowVector
            sx, sy, si = mi355slam.feature_search_sort(kps[f]["x"], kps[f]["y"])
            assert same_bits(r["sorted_x"], sx) and same_bits(r["sorted_y"], sy) and same_bits(r["sorted_idx"], si) and same_bits(r["kp_track"], kps[f]["track_id"])
            assert same_bits(r["word"], words[f]["word"]) and same_bits(r["weight"], words[f]["weight"]) and (r["weight"] == 0).any()
        state = dev.state()                                  # both slots, the pool and the poses after the two calls; slot 2 and every canary untouched
        for k in R.TABLES:
            assert same_bits(state[k], want[k]), k
        depths = state["kp_depth"][0, :n[0]]
        assert (depths == -1).sum() == 0 and len(np.unique(depths)) > 100      # every keypoint is inside the image: a track's depth or a sample

        # the triangulation matcher on admitted and on host-built keyframes
        built = [host_built(ctx, kps[f], words[f]) for f in range(2)]
        R1, t1, R2, t2 = np.eye(3), np.zeros(3), np.eye(3), np.array([0.3, 0.02, 0.01])
        E = mi355slam.create_E21(R1, t1, R2, t2)
        sf = mi355slam.scale_factors(8, 1.2)
        a = mi355slam.match_triangulation(ctx, [frames[1].on_device()], [frames[0].on_device()], E, sf, 2.0)
        b = mi355slam.match_triangulation(ctx, [built[1]], [built[0]], E, sf, 2.0)
        assert a[0][0] == b[0][0] > 50 and same_bits(a[1][0], b[1][0])
        print("triangulation matches on admitted and host-built keyframes: %d" % a[0][0])

        # the radius search on the admitted sorted arrays and on the host-sorted upload
        nq = 300
        qx, qy, qr = kps[0]["x"][:nq] + 1.5, kps[0]["y"][:nq] - 0.5, np.full(nq, 12.0, np.float32)
        ref_out = mi355slam.projection_topk(ctx, kps[1]["x"], kps[1]["y"], kps[1]["desc"], qx, qy, qr, kps[0]["desc"][:nq], t_octave=kps[1]["octave"])
        fb = frames[1].bufs
        dq = [ctx.upload(np.ascontiguousarray(v)) for v in (qx.astype(np.float32), qy.astype(np.float32), qr, kps[0]["desc"][:nq])]
        outs = [ctx.alloc(16 * nq + 16), ctx.alloc(8 * nq + 16), ctx.alloc(16 * nq + 16), ctx.alloc(4 * nq + 16), ctx.alloc(4 * nq + 16)]
        vp = mi355slam._vp
        ctx.check(mi355slam.lib().ms_projection_topk(ctx._h, vp(fb["sorted_x"]), vp(fb["sorted_y"]), vp(fb["sorted_idx"]), n[1], vp(fb["desc"]), vp(fb["octave"]), None,
                                                     vp(dq[0]), vp(dq[1]), vp(dq[2]), None, None, vp(dq[3]), nq, *[vp(o) for o in outs]), "ms_projection_topk")
        ctx.sync()
        mine = (outs[0].download(np.int32, (nq, 4)), outs[1].download(np.uint16, (nq, 4)), outs[2].download(np.int32, (nq, 4)), outs[3].download(np.int32, (nq,)),
                outs[4].download(np.int32, (nq,)))
        assert all(same_bits(x, y) for x, y in zip(mine, ref_out)) and mine[4].sum() > nq

        # ms_match_tracked on the admitted slot and on an uploaded one
        outcomes = []
        for admitted in (True, False):
            if admitted:
                kt = mi355slam.KeyframeTable(ctx, state["kf_mp"]); kp = mi355slam.KeypointTable(ctx, state["kp_x"], state["kp_y"], state["kp_octave"], state["kp_depth"])
                pool, kp_track = dev.tab["desc_pool"], res[1]["kp_track"]
            else:
                blank = {k: tables[k].copy() for k in ("kp_x", "kp_y", "kp_octave", "kp_depth", "desc_pool")}
                blank["kp_x"][1, :n[1]], blank["kp_y"][1, :n[1]], blank["kp_octave"][1, :n[1]] = kps[1]["x"], kps[1]["y"], kps[1]["octave"]
                blank["desc_pool"][base[1]:base[1] + n[1]] = kps[1]["desc"]
                kt = mi355slam.KeyframeTable(ctx, tables["kf_mp"]); kp = mi355slam.KeypointTable(ctx, blank["kp_x"], blank["kp_y"], blank["kp_octave"], blank["kp_depth"])
                pool, kp_track = ctx.upload(blank["desc_pool"]), kps[1]["track_id"]
            n_mp = 100
            table = mi355slam.MapPointTable(ctx, np.zeros((n_mp, 3)), np.zeros((n_mp, 3), np.float32), np.zeros(n_mp, np.float32), np.ones(n_mp, np.float32), np.zeros((n_mp, 8), np.uint32))
            tracks = mi355slam.TrackTable(ctx, np.full(n_mp, -1), np.full(200, -1), 250)
            flags, live = ctx.upload(np.zeros(n_mp, np.uint8)), ctx.upload(np.zeros(n_mp, np.uint8))
            out = dict(outcome=ctx.alloc(n[1]), created_rows=ctx.alloc(4 * n_mp), created_kp=ctx.alloc(4 * n_mp))
            frame = dict(slot=1, pose=POSE + 1, cam=CAM6, focal=520, desc_base=base[1], level_sigma_sq=mi355slam.level_sigma_sq(8, 1.2), rel_reprojection_threshold=0.05)
            pool.shape = (dev.n_pool, 8)
            rc, counts = kt.match_tracked_device(table, flags, live, tracks, kp, pool, frame, kp_track, np.arange(n_mp, dtype=np.int32), out)
            assert rc == 0, mi355slam.lib().ms_last_error(ctx._h)
            outcomes.append((counts, out["outcome"].download(np.uint8, (n[1],)), out["created_kp"].download(np.int32, (int(counts[0]),)),
                             table.desc.download(np.uint32, (n_mp, 8)), kt.download()[1]))
        assert outcomes[0][0][0] == (kps[1]["track_id"] >= 0).sum() > 20
        assert all(same_bits(x, y) for x, y in zip(*outcomes))
    finally:
        dev.free(); d_image.free()
        for fr in frames:
            fr.free()


# ---- 2. synthetic views
def plain_args(slot=1, desc_base=3, **kw):
    return dict(dict(slot=slot, desc_base=desc_base, pose=POSE), **kw)


@pytest.mark.parametrize("n, stride", [(0, 8), (1, 1), (257, 300), (640, 640)])
def test_sizes_at_which_a_path_changes(ctx, n, stride):
    frame = R.synth_frame(n, 40 + n, n_tracked=min(n, 5))
    tables = R.empty_tables(3, stride, stride + 9, n)
    vocab = device_vocab(ctx, "ragged")
    ids, depth = np.array([104, 100, 101, 102, 103, 100], np.int32), np.array([1, 2, 3, np.nan, -1, 6], np.float32)
    want, _ = admit_and_check(ctx, frame, tables, max(n, 1), plain_args(levels_up=2, track_ids=ids, track_depth=depth), vocab, (n, stride))
    assert want["rc"] == 0 and want["counts"][0] == n and (n < 2 or want["counts"][1] > 1)
    assert (want["kf_mp"][1] == -1).all() and same_bits(want["kf_pose"][1], POSE)


def test_ties_in_y_across_a_workgroup_boundary(ctx):
    frame = R.synth_frame(700, 7, y_step=60.0)               # 8 distinct y over 700 keypoints: equal values on both sides of lanes 255 | 256 and 511 | 512
    frame["y"][250:262] = 120.0
    frame["y"][300], frame["y"][301] = -0.0, 0.0             # equal: the index decides
    assert len(np.unique(frame["y"])) <= 9
    want, _ = admit_and_check(ctx, frame, R.empty_tables(2, 701, 800, 3), 700, plain_args())
    assert want["counts"].tolist() == [700, 0, 0]            # no vocabulary: no node lists
    idx = want["sorted_idx"][:700]
    assert (np.diff(idx)[np.diff(want["sorted_y"][:700]) == 0] > 0).all()


def test_one_node_then_six_hundred_nodes_and_stop_words(ctx):
    vocab, arrays = device_vocab(ctx, "wide"), vocab_arrays("wide")
    leaves = np.flatnonzero(arrays["word"] >= 0)
    frame = R.synth_frame(900, 12)
    frame["desc"] = arrays["desc"][leaves[:900]].copy()      # each keypoint sits on a leaf of its own
    tables = R.empty_tables(2, 900, 905, 4)
    want, _ = admit_and_check(ctx, frame, tables, 900, plain_args(levels_up=3), vocab, "one node")      # the node 3 levels up is the root
    kept = int((arrays["weight"][leaves[:900]] > 0).sum())
    assert 0 < kept < 900 and want["counts"].tolist() == [900, 1, kept] and want["node_id"][0] == 0      # stop words are in no list
    want, _ = admit_and_check(ctx, frame, tables, 900, plain_args(levels_up=0), vocab, "600 nodes", twice=False)
    assert want["counts"][1] >= 600 and want["counts"][2] == kept                                        # more heads than three trips of 256 pack
    assert (np.diff(want["node_start"][:want["counts"][1] + 1]) >= 1).all()


def test_every_source_of_a_depth(ctx):
    frame = R.synth_frame(6, 4, n_tracked=4)
    frame["x"][:], frame["y"][:] = [3.0, 3.4, 2.5, 3.5, 639.6, 5.0], [1.0, 1.0, 0.5, 1.5, 2.0, 479.5]
    image = np.arange(480 * 640, dtype=np.float32).reshape(480, 640)
    ids, depth = np.array([100, 101, 102, 103], np.int32), np.array([4.5, -2.0, np.nan, -0.0], np.float32)
    tables = R.empty_tables(2, 8, 20, 5)
    want, _ = admit_and_check(ctx, frame, tables, 6, plain_args(track_ids=ids, track_depth=depth, image=image), label="track and image")
    d = want["kp_depth"][1, :6]
    # the track | the track's is negative: the image | a NaN stays | -0.0 is not below 0 | column 640 and row 480 are outside
    assert d[0] == 4.5 and d[1] == image[1, 3] and np.isnan(d[2]) and d[3] == 0 and d[4] == -1 and d[5] == -1
    want, _ = admit_and_check(ctx, frame, tables, 6, plain_args(image=image), label="image alone", twice=False)
    assert want["kp_depth"][1, :6].tolist() == [image[1, 3], image[1, 3], image[0, 2], image[2, 4], -1.0, -1.0]
    want, _ = admit_and_check(ctx, frame, tables, 6, plain_args(track_ids=ids, track_depth=depth), label="tracks alone", twice=False)
    assert want["kp_depth"][1, 1] == -1 and want["kp_depth"][1, 5] == -1
    want, _ = admit_and_check(ctx, frame, tables, 6, plain_args(), label="neither", twice=False)
    assert (want["kp_depth"][1, :6] == -1).all()


# ---- 3. every refusal, with all bytes untouched
def test_capacity_refusals_report_n_and_the_call_then_succeeds_with_room(ctx):
    frame = R.synth_frame(40, 6)
    for label, stride, cap, n_pool in (("n = stride + 1", 39, 40, 60), ("cap_kp one short", 40, 39, 60), ("the pool one short", 40, 40, 42)):
        tables = R.empty_tables(2, stride, n_pool, 6)
        want, (rc, counts, _, _) = admit_and_check(ctx, frame, tables, cap, plain_args(), label=label, twice=False)
        assert rc == mi355slam.MS_ERR_CAPACITY and counts.tolist() == [40, 0, 0] and "40 keypoints" in mi355slam.lib().ms_last_error(ctx._h).decode(), label
        room = R.empty_tables(2, 40, 43, 6)
        want, (rc, counts, _, _) = admit_and_check(ctx, frame, room, 40, plain_args(), label=label + ", then room", twice=False)
        assert rc == 0 and counts[0] == 40


def test_invalid_views_and_rows_are_refused_before_any_write(ctx):
    frame = R.synth_frame(300, 9, n_tracked=10)
    tables = R.empty_tables(2, 300, 320, 7)
    message = lambda: mi355slam.lib().ms_last_error(ctx._h).decode()
    for j, name, value in ((299, "x", np.nan), (0, "y", np.inf), (256, "y", -np.inf)):
        bad = dict(frame)
        bad[name] = frame[name].copy()
        bad[name][j] = value
        want, (rc, counts, _, _) = admit_and_check(ctx, bad, tables, 300, plain_args(), label=(name, j), twice=False)
        assert rc == mi355slam.MS_ERR_INVALID and "1 of 300 keypoints have a coordinate that is not finite" in message()
    bound = {k: v.copy() for k, v in tables.items()}
    bound["kf_mp"][1, 299], bound["kf_mp"][1, 3], bound["kf_mp"][0, 5] = 49, 50, 7      # one valid entry in the row; 50 is not valid with n_mp = 50; slot 0 is another row
    want, (rc, counts, _, _) = admit_and_check(ctx, frame, bound, 300, plain_args(), label="a bound row", twice=False)
    assert rc == mi355slam.MS_ERR_INVALID and "slot 1 is not empty, 1 of its entries" in message()
    shorter = R.synth_frame(100, 9)                          # the valid entry lies behind n: the row is the slot's whole row
    want, (rc, _, _, _) = admit_and_check(ctx, shorter, bound, 300, plain_args(), label="bound behind n", twice=False)
    assert rc == mi355slam.MS_ERR_INVALID
    ids = np.array([100, 101, 102, 103, 104, 105, 106, 107, 108], np.int32)      # 109 is not listed
    want, (rc, _, _, _) = admit_and_check(ctx, frame, tables, 300, plain_args(track_ids=ids, track_depth=np.ones(9, np.float32)), label="an unlisted id", twice=False)
    assert rc == mi355slam.MS_ERR_INVALID and "1 tracked keypoints have an id that is not in track_ids" in message()
    want, (rc, _, _, _) = admit_and_check(ctx, frame, tables, 300, plain_args(), label="more than the view holds", capacity=299, twice=False)
    assert rc == mi355slam.MS_ERR_INVALID and "counts 300 keypoints in frame 1, its capacity is 299" in message()


def test_host_validation_runs_before_the_device(ctx):
    frame, tables = R.synth_frame(20, 3), R.empty_tables(2, 20, 30, 8)
    dev = Dev(ctx, tables, 20, frame)
    try:
        for kw in (dict(slot=2), dict(desc_base=31), dict(pose=np.full(12, np.nan)), dict(cam=(0.0, 1.0, 0.0, 0.0, 640, 480))):
            rc, counts, got = dev.call(dict(plain_args(cam=CAM6), **kw))
            assert rc == mi355slam.MS_ERR_INVALID and (counts == -77).all(), kw          # nothing written, counts included
        check(dev, 0, np.array([20, 0, 0]), {}, dict(tables, **dev.before, rc=0, counts=np.array([20, 0, 0])))
    finally:
        dev.free()


# ---- 4. and 5.
def test_nothing_is_allocated_after_warm_up_and_usable_is_the_unbound_mask(ctx):
    lib = mi355slam.lib()
    lib.ms_debug_host_allocs.restype = C.c_longlong
    vocab = device_vocab(ctx, "ragged")
    frame = R.synth_frame(500, 13, n_tracked=30)
    stride, n_slots = 512, 4
    t = R.empty_tables(n_slots, stride, 4 * 500, 9)
    kt = mi355slam.KeyframeTable(ctx, t["kf_mp"]); kp = mi355slam.KeypointTable(ctx, t["kp_x"], t["kp_y"], t["kp_octave"], t["kp_depth"])
    pool, poses = ctx.upload(t["desc_pool"]), mi355slam.KeyframePoseTable(ctx, t["kf_pose"])
    dev = Dev(ctx, R.empty_tables(1, 1, 1), 1, frame, capacity=520)      # the view alone is used
    out = mi355slam.AdmitFrame(ctx, 512)
    ids, depth = np.arange(100, 130, dtype=np.int32), np.ones(30, np.float32)
    try:
        allocs = []
        for i in range(23):
            args = plain_args(slot=i % n_slots, desc_base=500 * (i % n_slots), cam=CAM6, vocab=vocab, levels_up=1, track_ids=ids, track_depth=depth)
            res = mi355slam.keyframe_admit(ctx, dev.view, 1, kt, 50, kp, pool, poses, args, out)
            allocs.append(lib.ms_debug_host_allocs())
            assert res["counts"][0] == 500 and out.n == 500 and out.n_nodes == res["counts"][1] > 5
        assert len(set(allocs[3:])) == 1, allocs             # flat over 20 calls after three warm-ups
        mask = ctx.alloc(512)
        kt.unbound_mask([22 % n_slots], [500], 50, [mask])   # the slot of the last call
        ctx.sync()
        assert same_bits(mask.download(np.uint8, (500,)), out.download()["usable"][:500]) and (kt.download()[22 % n_slots] == -1).all()
        mask.free()
    finally:
        dev.free(); out.free(); kp.free(); kt.kf_mp.free(); pool.free(); poses.pose.free()
