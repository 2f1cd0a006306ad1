"""The front end's chain as a chain, on the device: the schedule of tests/frame_chain_ref.py -- the extract, three publishes,
six tracker frames of admit / match / pose solve / finish, the removal of the oldest keyframe, a second extract into the tables as they
then are -- in one context on ONE set of device tables.  The tables go up once; afterwards only what the real chain uploads goes up (the
feature block, the remove list, kf_list, the changed source before the second extract).

After EVERY call every table of the set comes down, the ones the call must not touch included, and is compared bit for bit with the
composed restatement, as are the call's host outputs; a canary behind every device buffer is checked with every download.  The pose step
follows test_gpu_pose_tables.check_frame (the gathered problem and the solve against ms_ba_solve_host bit for bit, the result against
the CPU oracle with test_gpu_ba._check's bar); the restatement continues from the device's pose bytes, so no later comparison is widened.
The invariants I1 - I5 and the n_obs promises of frame_chain_ref are held on the downloaded state after every call.  The match goes
through the two halves of KeyframeTable.match_tracked (match_tracked_bind, match_tracked_refresh: tracked_rows / checked_rows stay on the
device between them) with a download in between; ms_observation_count through the C entry point on the tables' own n_obs, because the
binding's method allocates its outputs and brings them down.

The schedule runs twice in the context, the second pass from re-uploaded initial tables on the workspaces the first pass left dirty:
every downloaded byte and every host output identical, ms_debug_host_allocs (which counts the library's host blocks AND its device
workspaces) flat across the second pass.  The scene's conditions are asserted in tests/test_frame_chain_ref.py."""
import ctypes as C

import numpy as np
import pytest

import frame_chain_ref as R
import map_extract_ref as ME
import mi355slam
import pose_tables_ref as PT
from test_gpu_pose_tables import check_frame, gathered_equal

pytestmark = pytest.mark.gpu
CANARY, PAD, FILL = 0xA5, 64, 0x5A
N_KF, STRIDE = R.N_DST_KF, R.STRIDE


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def with_canary(a):
    return np.concatenate([np.ascontiguousarray(a).view(np.uint8).reshape(-1), np.full(PAD, CANARY, np.uint8)])


def put(ctx, buf, arr):
    arr = np.ascontiguousarray(arr)
    ctx.check(mi355slam.lib().ms_dev_upload(ctx._h, C.c_void_p(buf.ptr), mi355slam._vp(arr), C.c_size_t(arr.nbytes)), "ms_dev_upload")


def wrap(cls, **fields):
    """A binding object over buffers that are on the device already."""
    o = cls.__new__(cls)
    for k, v in fields.items():
        setattr(o, k, v)
    return o


class Device:
    """The source tables, the destination tables, the record and the rasters on the device, a canary behind each; allocated once."""

    def __init__(self, ctx, w):
        self.ctx, self.w = ctx, w
        st0 = R.initial_state(w, FILL)
        self.n_mp = st0["n_mp"]
        self.names = R.device_names(st0)
        self.like = {k: st0[k] for k in self.names}
        self.dst = {k: ctx.upload(with_canary(st0[k])) for k in self.names}
        self.src_names = [k for k in mi355slam.MAP_EXTRACT_SRC if w["src"].get(k) is not None]
        self.src = {k: ctx.upload(with_canary(w["src"][k])) for k in self.src_names}
        self.src_now = w["src"]
        self.fixed = dict(image=w["image"], mask=w["mask"], local_rows=w["local_rows"])
        self.aux = {k: ctx.upload(with_canary(v)) for k, v in self.fixed.items()}
        d = self.dst
        self.kt = wrap(mi355slam.KeyframeTable, ctx=ctx, kf_mp=d["kf_mp"], n_kf=N_KF, stride=STRIDE)
        self.src_kt = wrap(mi355slam.KeyframeTable, ctx=ctx, kf_mp=self.src["kf_mp"], n_kf=R.N_SRC_KF, stride=STRIDE)
        self.table = wrap(mi355slam.MapPointTable, ctx=ctx, n=self.n_mp, pos=d["mp_pos"], norm=d["mp_norm"], min_dist=d["mp_min_dist"], max_dist=d["mp_max_dist"], desc=d["mp_desc"])
        self.kp = wrap(mi355slam.KeypointTable, ctx=ctx, n_kf=N_KF, stride=STRIDE, x=d["kp_x"], y=d["kp_y"], octave=d["kp_octave"], depth=d["kp_depth"])
        self.tracks = wrap(mi355slam.TrackTable, ctx=ctx, track_base=R.TRACK_BASE, n_mp=self.n_mp, n_track=R.N_TRACK, mp_track=d["mp_track"], track_row=d["track_row"])
        self.poses = wrap(mi355slam.KeyframePoseTable, ctx=ctx, n=N_KF, pose=d["kf_pose"])
        self.pool = d["desc_pool"]
        self.pool.shape = (w["pool_dst"], 8)
        self.adj = mi355slam.PoseAdjuster(ctx, STRIDE, PT.W.sigma_levels())          # ONE persistent handle for both passes

    def upload_initial(self):
        """The tables as they are before the first extract; nothing is allocated."""
        st0 = R.initial_state(self.w, FILL)
        for k in self.names:
            put(self.ctx, self.dst[k], st0[k])
        self.upload_source(self.w["src"])

    def upload_source(self, src):
        for k in self.src_names:
            put(self.ctx, self.src[k], src[k])
        self.src_now = src

    def _down(self, buf, like, label):
        raw = buf.download(np.uint8, (like.nbytes + PAD,))
        assert (raw[like.nbytes:] == CANARY).all(), ("canary", label)
        return raw[:like.nbytes].view(like.dtype).reshape(like.shape)

    def state(self, label=""):
        """Every destination table and the record, each canary checked."""
        return {k: self._down(self.dst[k], self.like[k], (label, k)) for k in self.names}

    def others_untouched(self, label=""):
        """The source tables and the rasters hold what was uploaded."""
        for k in self.src_names:
            assert same_bits(self._down(self.src[k], self.src_now[k], (label, k)), np.asarray(self.src_now[k])), (label, "source", k)
        for k, v in self.fixed.items():
            assert same_bits(self._down(self.aux[k], v, (label, k)), v), (label, k)

    def free(self):
        self.adj.close()
        for b in list(self.dst.values()) + list(self.src.values()) + list(self.aux.values()):
            b.free()


def host_allocs():
    f = mi355slam.lib().ms_debug_host_allocs
    f.restype = C.c_longlong
    return f()


def device_step(d, st, step, run, fx):
    """The device call of one step.  st: the restated state BEFORE the step (the host's kf_id and desc_base are read from it);
    fx: what the frame's earlier device calls left.  Returns the call's host outputs."""
    ctx, w, (name, arg) = d.ctx, d.w, step
    err = lambda: mi355slam.lib().ms_last_error(ctx._h)
    if name == "source_change":
        d.upload_source(w["src2"])
        return {}
    if name == "extract":
        src, active = d.src_now, w["active%d" % arg]
        rc, out = d.src_kt.map_extract_device({k: v for k, v in d.src.items() if k != "kf_mp"}, {k: d.dst[k] for k in ME.dst_names(src)}, R.sizes(w, src), src["kf_id"], active,
                                              src["desc_base"], np.take(src["n_kp"], active))
        assert rc == 0, (step, rc, err())
        return out
    if name == "counts":                                     # the C entry point on the table's own n_obs: the binding's form allocates its outputs and brings them down
        kf_id = np.ascontiguousarray(st["kf_id"], np.int32)
        rc = mi355slam.lib().ms_observation_count(ctx._h, mi355slam._vp(d.dst["kf_mp"]), N_KF, STRIDE, d.n_mp, mi355slam._vp(kf_id), mi355slam._vp(d.dst["n_obs"]), None, None)
        assert rc == 0, (step, rc, err())
        return {}
    if name == "publish":
        kf_list = [s for s in range(N_KF) if st["kf_id"][s] >= 0]
        tables = dict({k: d.dst[k] for k in ("mp_pos", "mp_norm", "mp_flags", "mp_live", "n_obs", "kf_mp", "kf_pose", "rec_pos", "rec_state")}, mp_color=None, local_rows=d.aux["local_rows"])
        rc, out = mi355slam.map_publish_device(ctx, tables, d.n_mp, N_KF, STRIDE, len(w["local_rows"]),
                                               dict(what=mi355slam.MS_PUBLISH_VIEW | mi355slam.MS_PUBLISH_RECORD, current_slot=arg, min_record_obs=R.MIN_RECORD_OBS), kf_list)
        assert rc == 0, (step, rc, err())
        return out
    if name == "remove":
        rc, out = d.kt.frame_finish_device(d.dst["mp_flags"], d.dst["mp_live"], d.table, d.dst["mp_track"], d.dst["n_obs"], st["kf_id"], arg, -1, 0)
        assert rc == 0, (step, rc, err())
        return out
    fr = w["frames"][arg]
    if name == "admit":
        args = dict(slot=fr["slot"], pose=fr["pose"], depth_image=d.aux["image"], depth_width=640, depth_height=480, valid_mask=d.aux["mask"], mask_width=640, mask_height=480)
        rc, out = mi355slam.frame_admit_device(ctx, {k: d.dst[k] for k in mi355slam.FRAME_ADMIT_TABLES}, N_KF, STRIDE, d.n_mp, fr["feat"], args)
        assert rc == 0, (step, rc, err())
        fx["kp_track"] = out["kp_track"]
        return out
    if name == "bind":                                       # the first half of KeyframeTable.match_tracked
        frame = dict(slot=fr["slot"], pose=fr["pose"], kp_track=fx["kp_track"])
        assert frame["kp_track"] is fx["kp_track"]           # the admit's array, untouched
        res = d.kt.match_tracked_bind(d.table, d.dst["mp_flags"], d.dst["mp_live"], d.tracks, d.kp, d.pool, d.poses, st["kf_id"], st["cams"], st["focal"], st["desc_base"], frame,
                                      np.zeros(0, np.int32), R.SETTINGS, R.VIEW_COS_LIMIT)
        fx["match"] = res
        some = lambda k, n: res["bufs"][k].download(np.int32, (n,)) if n else np.zeros(0, np.int32)
        return dict(outcome=res["outcome"], counts=np.asarray(res["counts"]), created_rows=res["created_rows"], created_kp=res["created_kp"], status=res["status"],
                    tracked_rows=some("tracked_rows", int(res["counts"][1])), checked_rows=some("checked_rows", int(res["counts"][2])))
    if name == "refresh":                                    # the second half; tracked_rows / checked_rows never left the device
        res = d.kt.match_tracked_refresh(fx.pop("match"), R.MR.scale_factors())
        return dict(refresh_rows=res["refresh_rows"])
    if name == "pose":
        frame = R.pose_frame(fr, len(fx["kp_track"]))
        rc, res = d.adj.solve_device(d.kt, d.dst["mp_flags"], d.dst["mp_live"], d.table, d.kp, d.poses, frame, True)
        assert rc == 0, (step, rc, err())
        fx["problem"] = d.adj.problem()
        return dict(rc=rc, res=res, problem=fx["problem"])
    if name == "finish":
        remove = [] if fr["stays"] else [fr["slot"]]
        rc, out = d.kt.frame_finish_device(d.dst["mp_flags"], d.dst["mp_live"], d.table, d.dst["mp_track"], d.dst["n_obs"], st["kf_id"], remove, fr["slot"], len(fx["kp_track"]))
        assert rc == 0, (step, rc, err())
        return out
    raise ValueError(name)


def outputs_of(name):
    """The host outputs of a step that are compared with the restatement's, bit for bit."""
    pub = tuple(k for k, _, _ in mi355slam.MAP_PUBLISH_PUB + mi355slam.MAP_PUBLISH_EV)
    cloud = ("cloud_row", "cloud_kp", "cloud_track", "cloud_pos", "removed_rows", "counts")
    return dict(extract=("counts", "dst_desc_base"), publish=("counts", "pose_wc") + pub, admit=("counts", "kp_track", "kp_feature"),
                bind=("outcome", "counts", "created_rows", "created_kp", "tracked_rows", "checked_rows", "status"), refresh=("refresh_rows",), finish=cloud, remove=cloud).get(name, ())


def bytes_of(v):
    return np.ascontiguousarray(v).tobytes()


def run_pass(d, ctx, oracle, verify_solver):
    """The schedule once.  Returns every downloaded byte and every host output, in order."""
    w = d.w
    st, run, seen = R.initial_state(w, FILL), {}, []
    got = d.state("initial")
    for k in d.names:
        assert same_bits(got[k], st[k]), ("initial", k)
    frames = {}
    for i, step in enumerate(R.schedule()):
        name, arg = step
        label = "step %d %s" % (i, step)
        fx = frames.setdefault(arg, {}) if name in ("admit", "bind", "refresh", "pose", "finish") else {}
        before = R.pose_scene(st) if name == "pose" else None
        out = device_step(d, st, step, run, fx)
        if name == "pose":                                   # the restatement continues from the device's pose bytes (C7)
            want = R.apply_step(st, w, step, run, solve=lambda prob, frame, g: out["res"]["pose"])
        else:
            want = R.apply_step(st, w, step, run)
        # ---- the host outputs
        for k in outputs_of(name):
            a, b = np.asarray(out[k]), np.asarray(want[k])
            assert a.shape == b.shape and bytes_of(a.astype(b.dtype) if a.dtype.kind == b.dtype.kind == "i" else a) == bytes_of(b), (label, k, a, b)
            seen.append((label, k, bytes_of(a)))
        # ---- every table, the untouched ones included
        got = d.state(label)
        for k in d.names:
            assert same_bits(got[k], st[k]), (label, k, np.flatnonzero(got[k].reshape(-1) != st[k].reshape(-1))[:8])
        seen += [(label, k, got[k].tobytes()) for k in d.names]
        # ---- the pose step as test_gpu_pose_tables.check_frame has it
        if name == "pose":
            p = want
            gathered_equal(out["problem"], p["g"])
            assert out["res"]["ran"] == p["ran"] and out["res"]["n_triangulated"] == p["g"]["n"], label
            seen.append((label, "pose", bytes_of(out["res"]["pose"]) + bytes_of(out["res"]["chi2"])))
            if verify_solver:
                after = dict(kf_mp=got["kf_mp"], mp_flags=got["mp_flags"], mp_live=got["mp_live"], mp_pos=got["mp_pos"], poses=got["kf_pose"])
                check_frame(ctx, oracle, before, p["frame"], p["g"], out["rc"], out["res"], out["problem"], after, label)
        # ---- the cross-step identities, device against device
        if name == "finish":
            prob = fx["problem"]
            assert same_bits(out["cloud_pos"], prob["point"]), label                                      # the cloud IS the point array of the frame's gather
            kept = run[("frame", arg)]["pose"]["g"]["kept"]
            assert same_bits(out["cloud_kp"], kept.astype(np.int32)) and same_bits(out["cloud_row"], frames[arg]["rows_at_pose"][kept]), label
        if name == "pose":
            fx["rows_at_pose"] = got["kf_mp"][w["frames"][arg]["slot"]].copy()
        # ---- the invariants and the n_obs promises on the DEVICE state
        dev = dict(got, kf_id=st["kf_id"], n_mp=st["n_mp"], track_base=st["track_base"])
        R.check_invariants(dev, label)
        R.check_n_obs(dev, step, want, label)
        if name == "finish":
            d.others_untouched(label)                        # at the end of each frame: the source, the rasters, the local list
    return seen


@pytest.fixture(scope="module")
def device(ctx):
    d = Device(ctx, R.world())
    yield d
    d.free()


def test_the_schedule_twice_on_one_set_of_tables(ctx, oracle, device):
    d = device
    d.upload_initial()
    first = run_pass(d, ctx, oracle, verify_solver=True)
    d.upload_initial()                                       # the second pass: the same tables again, the workspaces as the first pass left them
    before = host_allocs()
    second = run_pass(d, ctx, oracle, verify_solver=False)   # (ms_ba_solve_host and the oracle are the first pass's checks: they allocate)
    assert host_allocs() == before, (before, host_allocs())
    assert len(first) == len(second)
    for a, b in zip(first, second):
        assert a[:2] == b[:2] and a[2] == b[2], a[:2]
    n_bytes = sum(len(x[2]) for x in first)
    print("%d steps, %d compared arrays, %.1f MB per pass" % (len(R.schedule()), len(first), n_bytes / 1e6))
