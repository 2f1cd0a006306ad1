"""ctypes loader for the CPU oracle (oracle/libmso.so).

TEST INFRASTRUCTURE ONLY.  Importable from tests/, __graft_entry__.smoke() and bench.py's
cpu_baseline leg; the product package (slam-module_amd/) must never import this module.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

MAX_LEVELS = 16
u8p = C.POINTER(C.c_uint8)
i32p = C.POINTER(C.c_int32)
u32p = C.POINTER(C.c_uint32)
u16p = C.POINTER(C.c_uint16)
f32p = C.POINTER(C.c_float)
f64p = C.POINTER(C.c_double)


class OrbConfig(C.Structure):
    _fields_ = [("levels", C.c_int), ("scale_factor", C.c_float), ("max_kpts", C.c_int),
                ("lk_track_level", C.c_int), ("fast_threshold", C.c_int), ("min_distance", C.c_float)]


class Keypoints(C.Structure):
    _fields_ = [("n", C.c_int), ("x", f32p), ("y", f32p), ("angle", f32p), ("octave", i32p),
                ("desc", u32p), ("track_id", i32p)]


class Pyramid(C.Structure):
    _fields_ = [("levels", C.c_int), ("w", C.c_int * MAX_LEVELS), ("h", C.c_int * MAX_LEVELS),
                ("img", u8p * MAX_LEVELS), ("blur", u8p * MAX_LEVELS)]


class Bow(C.Structure):
    _fields_ = [("n_nodes", C.c_int), ("node_id", i32p), ("node_start", i32p), ("kp_idx", i32p)]


def build():
    subprocess.check_call(["make", "-s", "-C", _HERE, "libmso.so"])


def lib():
    global _LIB
    if _LIB is None:
        path = os.path.join(_HERE, "libmso.so")
        if not os.path.exists(path):
            build()
        _LIB = C.CDLL(path)
        _LIB.mso_fast_atan2.restype = C.c_float
        _LIB.mso_fast_atan2.argtypes = [C.c_float, C.c_float]
        _LIB.mso_cos.restype = C.c_float
        _LIB.mso_cos.argtypes = [C.c_float]
        _LIB.mso_sin.restype = C.c_float
        _LIB.mso_sin.argtypes = [C.c_float]
        _LIB.mso_ic_angle.restype = C.c_float
        _LIB.mso_hamming256.restype = C.c_uint
    return _LIB


def _p(a, t):
    return a.ctypes.data_as(t) if a is not None else None


def cfg(levels=8, scale_factor=1.2, max_kpts=2000, lk_track_level=0, fast_threshold=20, min_distance=0.0):
    return OrbConfig(levels, scale_factor, max_kpts, lk_track_level, fast_threshold, min_distance)


# ---- geometry ----
def scale_factors(levels, f):
    out = np.zeros(levels, np.float32)
    lib().mso_scale_factors(levels, C.c_float(f), _p(out, f32p))
    return out


def level_sigma_sq(levels, f):
    out = np.zeros(levels, np.float32)
    lib().mso_level_sigma_sq(levels, C.c_float(f), _p(out, f32p))
    return out


def level_quotas(levels, f, max_kpts):
    out = np.zeros(levels, np.int32)
    lib().mso_level_quotas(levels, C.c_float(f), max_kpts, _p(out, i32p))
    return out


def level_sizes(levels, f, w, h):
    ws = np.zeros(levels, np.int32)
    hs = np.zeros(levels, np.int32)
    lib().mso_level_sizes(levels, C.c_float(f), w, h, _p(ws, i32p), _p(hs, i32p))
    return ws, hs


def umax():
    out = np.zeros(16, np.int32)
    lib().mso_umax(_p(out, i32p))
    return out


def gauss7_taps():
    out = np.zeros(7, np.int32)
    lib().mso_gauss7_derive(_p(out, i32p))
    fixed = np.array((C.c_int * 7).in_dll(lib(), "mso_gauss7_q8"), dtype=np.int32)
    return out, fixed


def pattern():
    return np.array((C.c_int8 * 1024).in_dll(lib(), "mso_orb_pattern"), dtype=np.int8)


# ---- pixels ----
def resize(src, dw, dh):
    src = np.ascontiguousarray(src, np.uint8)
    dst = np.zeros((dh, dw), np.uint8)
    lib().mso_resize_linear_u8(_p(src, u8p), src.shape[1], src.shape[0], src.shape[1], _p(dst, u8p), dw, dh, dw)
    return dst


def gauss7(src):
    src = np.ascontiguousarray(src, np.uint8)
    dst = np.zeros_like(src)
    lib().mso_gauss7_u8(_p(src, u8p), src.shape[1], src.shape[0], src.shape[1], _p(dst, u8p), src.shape[1])
    return dst


def build_pyramid(config, img):
    img = np.ascontiguousarray(img, np.uint8)
    P = Pyramid()
    rc = lib().mso_build_pyramid(C.byref(config), _p(img, u8p), img.shape[1], img.shape[0], img.shape[1], C.byref(P))
    assert rc == 0
    levels, blurs = [], []
    for l in range(P.levels):
        n = P.w[l] * P.h[l]
        levels.append(np.ctypeslib.as_array(P.img[l], shape=(n,)).reshape(P.h[l], P.w[l]).copy())
        blurs.append(np.ctypeslib.as_array(P.blur[l], shape=(n,)).reshape(P.h[l], P.w[l]).copy())
    lib().mso_free_pyramid(C.byref(P))
    return levels, blurs


def fast_score_map(img, threshold=0):
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape
    out = np.zeros((h, w), np.int32)
    L = lib()
    for y in range(3, h - 3):
        for x in range(3, w - 3):
            s = L.mso_fast_score(_p(img, u8p), w, x, y)
            out[y, x] = s if s > threshold else 0
    return out


def detect_level(img, threshold, quota, min_dist=0):
    img = np.ascontiguousarray(img, np.uint8)
    xs = np.zeros(quota + 1, np.int32)
    ys = np.zeros(quota + 1, np.int32)
    sc = np.zeros(quota + 1, np.int32)
    n = lib().mso_detect_level(_p(img, u8p), img.shape[1], img.shape[0], img.shape[1], threshold, quota, int(min_dist),
                               _p(xs, i32p), _p(ys, i32p), _p(sc, i32p))
    return xs[:n].copy(), ys[:n].copy(), sc[:n].copy()


def level_min_dist(g, w, h):
    return int(lib().mso_level_min_dist(C.c_float(g), int(w), int(h)))


def ic_angle(img, x, y):
    img = np.ascontiguousarray(img, np.uint8)
    return float(lib().mso_ic_angle(_p(img, u8p), img.shape[1], int(x), int(y)))


def orb_descriptor(blur, x, y, angle_deg):
    blur = np.ascontiguousarray(blur, np.uint8)
    d = np.zeros(8, np.uint32)
    lib().mso_orb_descriptor(_p(blur, u8p), blur.shape[1], int(x), int(y), C.c_float(angle_deg), _p(d, u32p))
    return d


def orb_extract(config, img, valid_mask=None, track_xy=None, track_id=None):
    img = np.ascontiguousarray(img, np.uint8)
    nt = 0 if track_xy is None else len(track_xy)
    cap = config.max_kpts + nt + 16          # the rounded per-level quotas can add up to a few more than max_kpts
    out = dict(x=np.zeros(cap, np.float32), y=np.zeros(cap, np.float32), angle=np.zeros(cap, np.float32),
               octave=np.zeros(cap, np.int32), desc=np.zeros((cap, 8), np.uint32), track_id=np.zeros(cap, np.int32))
    kp = Keypoints(0, _p(out["x"], f32p), _p(out["y"], f32p), _p(out["angle"], f32p), _p(out["octave"], i32p),
                   _p(out["desc"], u32p), _p(out["track_id"], i32p))
    txy = None if track_xy is None else np.ascontiguousarray(track_xy, np.float32)
    tid = None if track_id is None else np.ascontiguousarray(track_id, np.int32)
    vm = None if valid_mask is None else np.ascontiguousarray(valid_mask, np.uint8)
    n = lib().mso_orb_extract(C.byref(config), _p(img, u8p), img.shape[1], img.shape[0], img.shape[1], _p(vm, u8p),
                              _p(txy, f32p), _p(tid, i32p), nt, C.byref(kp), cap)
    assert n >= 0
    return {k: v[:n].copy() for k, v in out.items()}


def synth_frame(w, h, seed, shift_x=0, shift_y=0):
    img = np.zeros((h, w), np.uint8)
    lib().mso_synth_frame(_p(img, u8p), w, h, C.c_uint32(seed), shift_x, shift_y)
    return img


# ---- matching ----
def hamming256(a, b):
    a = np.ascontiguousarray(a, np.uint32)
    b = np.ascontiguousarray(b, np.uint32)
    return int(lib().mso_hamming256(_p(a, u32p), _p(b, u32p)))


def hamming_best2(q, t, q_bucket=None, t_bucket=None, t_valid=None):
    q = np.ascontiguousarray(q, np.uint32)
    t = np.ascontiguousarray(t, np.uint32)
    nq, nt = len(q), len(t)
    bi = np.zeros(nq, np.int32)
    bd = np.zeros(nq, np.uint16)
    sd = np.zeros(nq, np.uint16)
    qb = None if q_bucket is None else np.ascontiguousarray(q_bucket, np.int32)
    tb = None if t_bucket is None else np.ascontiguousarray(t_bucket, np.int32)
    tv = None if t_valid is None else np.ascontiguousarray(t_valid, np.uint8)
    lib().mso_hamming_best2(_p(q, u32p), nq, _p(t, u32p), nt, _p(qb, i32p), _p(tb, i32p), _p(tv, u8p),
                            _p(bi, i32p), _p(bd, u16p), _p(sd, u16p))
    return bi, bd, sd


def angle_check(delta, ids):
    delta = np.ascontiguousarray(delta, np.float32)
    ids = np.ascontiguousarray(ids, np.int32)
    inv = np.zeros(max(len(ids), 1), np.int32)
    m = lib().mso_angle_check(_p(delta, f32p), _p(ids, i32p), len(ids), _p(inv, i32p))
    return inv[:m].copy()


def best2_candidates(qdesc, tdesc, cand, skip=None, t_octave=None):
    q = np.ascontiguousarray(qdesc, np.uint32); t = np.ascontiguousarray(tdesc, np.uint32).reshape(-1, 8)
    c = np.ascontiguousarray(cand, np.int32)
    sk = None if skip is None else np.ascontiguousarray(skip, np.uint8)
    oc = None if t_octave is None else np.ascontiguousarray(t_octave, np.int32)
    best, second, bo, so = C.c_uint(), C.c_uint(), C.c_int(), C.c_int()
    bi = lib().mso_best2_candidates(_p(q, u32p), _p(t, u32p), _p(c, i32p), len(c), _p(sk, u8p), _p(oc, i32p),
                                    C.byref(best), C.byref(second), C.byref(bo), C.byref(so))
    return bi, best.value, second.value, bo.value, so.value


def features_around(sx, sy, x, y, r):
    """positions (in the y-sorted arrays) of the points within radius r, in the reference's output order"""
    sx = np.ascontiguousarray(sx, np.float32); sy = np.ascontiguousarray(sy, np.float32)
    out = np.zeros(len(sx), np.int32)
    lib().mso_features_around.restype = C.c_int
    n = lib().mso_features_around(_p(sx, f32p), _p(sy, f32p), len(sx), C.c_float(x), C.c_float(y), C.c_float(r), _p(out, i32p))
    return out[:n].copy()


def descriptor_medoid(desc):
    d = np.ascontiguousarray(desc, np.uint32).reshape(-1, 8)
    lib().mso_descriptor_medoid.restype = C.c_int
    return lib().mso_descriptor_medoid(_p(d, u32p), len(d))


def bow_transform(vocab, desc, levels_up=4):
    """vocab = dict(parent, desc, weight, word, depth_levels); returns word, weight, node per descriptor"""
    par = np.ascontiguousarray(vocab["parent"], np.int32); nd = np.ascontiguousarray(vocab["desc"], np.uint32).reshape(-1, 8)
    wt = np.ascontiguousarray(vocab["weight"], np.float64); wd = np.ascontiguousarray(vocab["word"], np.int32)
    d = np.ascontiguousarray(desc, np.uint32).reshape(-1, 8)
    n = len(d)
    word = np.zeros(n, np.int32); weight = np.zeros(n, np.float64); node = np.zeros(n, np.int32)
    lib().mso_bow_transform.restype = None
    lib().mso_bow_transform(len(par), _p(par, i32p), _p(nd, u32p), _p(wt, f64p), _p(wd, i32p), int(vocab["depth_levels"]),
                            _p(d, u32p), n, int(levels_up), _p(word, i32p), _p(weight, f64p), _p(node, i32p))
    return word, weight, node


def bow_assemble(word, weight, node):
    """BowVector (words, values) and FeatureVector (nodes, start, feat) the way DBoW2's std::maps iterate"""
    word = np.ascontiguousarray(word, np.int32); weight = np.ascontiguousarray(weight, np.float64); node = np.ascontiguousarray(node, np.int32)
    n = len(word)
    ow = np.zeros(n + 1, np.int32); ov = np.zeros(n + 1, np.float64); fn = np.zeros(n + 1, np.int32); fs = np.zeros(n + 2, np.int32); ff = np.zeros(n + 1, np.int32)
    nf = C.c_int(0)
    lib().mso_bow_assemble.restype = C.c_int
    nv = lib().mso_bow_assemble(_p(word, i32p), _p(weight, f64p), _p(node, i32p), n, _p(ow, i32p), _p(ov, f64p), _p(fn, i32p), _p(fs, i32p), _p(ff, i32p), C.byref(nf))
    return ow[:nv].copy(), ov[:nv].copy(), fn[:nf.value].copy(), fs[:nf.value + 1].copy(), ff[:fs[nf.value]].copy()


def make_bow(bucket_of_kp):
    """CSR over ascending node ids; keypoints of a node in ascending keypoint index (DBoW2 insertion order).
    A tuple (node_id, node_start, kp_idx) is taken as the CSR itself (tests with hand-made node lists)."""
    if isinstance(bucket_of_kp, tuple):
        ids, start, order = [np.ascontiguousarray(a, np.int32) for a in bucket_of_kp]
    else:
        bucket_of_kp = np.asarray(bucket_of_kp, np.int32)
        order = np.argsort(bucket_of_kp, kind="stable").astype(np.int32)
        ids, counts = np.unique(bucket_of_kp, return_counts=True)
        start = np.zeros(len(ids) + 1, np.int32)
        start[1:] = np.cumsum(counts)
    keep = dict(node_id=np.ascontiguousarray(ids, np.int32), node_start=start, kp_idx=order)
    b = Bow(len(ids), _p(keep["node_id"], i32p), _p(keep["node_start"], i32p), _p(keep["kp_idx"], i32p))
    return b, keep


def match_loop_closure(desc1, angle1, usable1, bucket1, desc2, angle2, usable2, bucket2, lowe_ratio, check_orientation=True):
    d1 = np.ascontiguousarray(desc1, np.uint32); d2 = np.ascontiguousarray(desc2, np.uint32)
    a1 = np.ascontiguousarray(angle1, np.float32); a2 = np.ascontiguousarray(angle2, np.float32)
    u1 = np.ascontiguousarray(usable1, np.uint8); u2 = np.ascontiguousarray(usable2, np.uint8)
    b1, k1 = make_bow(bucket1); b2, k2 = make_bow(bucket2)
    m = np.zeros(len(d1), np.int32)
    n = lib().mso_match_loop_closure(_p(d1, u32p), _p(a1, f32p), _p(u1, u8p), len(d1), C.byref(b1),
                                     _p(d2, u32p), _p(a2, f32p), _p(u2, u8p), len(d2), C.byref(b2),
                                     C.c_float(lowe_ratio), int(check_orientation), _p(m, i32p))
    return n, m


def create_E21(R1, t1, R2, t2):
    E = np.zeros(9, np.float64)
    R1 = np.ascontiguousarray(R1, np.float64); R2 = np.ascontiguousarray(R2, np.float64)
    t1 = np.ascontiguousarray(t1, np.float64); t2 = np.ascontiguousarray(t2, np.float64)
    lib().mso_create_E21(_p(R1, f64p), _p(t1, f64p), _p(R2, f64p), _p(t2, f64p), _p(E, f64p))
    return E.reshape(3, 3)


def match_triangulation(desc1, angle1, octave1, bearing1, usable1, bucket1,
                        desc2, angle2, bearing2, usable2, bucket2, E12, scale_factors_, thr_deg, check_orientation=True):
    d1 = np.ascontiguousarray(desc1, np.uint32); d2 = np.ascontiguousarray(desc2, np.uint32)
    a1 = np.ascontiguousarray(angle1, np.float32); a2 = np.ascontiguousarray(angle2, np.float32)
    o1 = np.ascontiguousarray(octave1, np.int32)
    be1 = np.ascontiguousarray(bearing1, np.float64); be2 = np.ascontiguousarray(bearing2, np.float64)
    u1 = np.ascontiguousarray(usable1, np.uint8); u2 = np.ascontiguousarray(usable2, np.uint8)
    E = np.ascontiguousarray(E12, np.float64); sf = np.ascontiguousarray(scale_factors_, np.float32)
    b1, k1 = make_bow(bucket1); b2, k2 = make_bow(bucket2)
    m = np.zeros(len(d1), np.int32)
    n = lib().mso_match_triangulation(_p(d1, u32p), _p(a1, f32p), _p(o1, i32p), _p(be1, f64p), _p(u1, u8p), len(d1), C.byref(b1),
                                      _p(d2, u32p), _p(a2, f32p), _p(be2, f64p), _p(u2, u8p), len(d2), C.byref(b2),
                                      _p(E, f64p), _p(sf, f32p), C.c_float(thr_deg), int(check_orientation), _p(m, i32p))
    return n, m


# ---- bundle adjustment ----
class BaProblem(C.Structure):
    _fields_ = [("n_pose", C.c_int), ("n_point", C.c_int), ("n_obs", C.c_int), ("n_edge", C.c_int),
                ("pose", f64p), ("pose_fixed", u8p), ("point", f64p), ("point_fixed", u8p),
                ("obs_pose", i32p), ("obs_point", i32p), ("obs_uv", f64p), ("obs_info", f64p), ("huber_delta", C.c_double),
                ("edge_i", i32p), ("edge_j", i32p), ("edge_meas", f64p), ("edge_info", f64p), ("max_iters", C.c_int)]


class BaStats(C.Structure):
    _fields_ = [("iters", C.c_int), ("trials_total", C.c_int), ("stop_reason", C.c_int),
                ("lambda_", C.c_double), ("chi2_init", C.c_double), ("chi2_final", C.c_double), ("min_abs_gain", C.c_double)]


def ba_solve(prob, max_iters=10, full_system=False, g2o_stale_chi2=False, force_reject=0):
    """prob: dict from tests/ba_synth.py (numpy arrays).  Returns dict(pose, point, chi2, stats).  g2o_stale_chi2: per-observation chi2 as g2o's edge->chi2() holds it
    after optimize() (the last trial's errors, even of a rejected trial); force_reject: the first n trials count as rejected (test hook, also in the GPU solver)."""
    pose = np.ascontiguousarray(prob["pose"], np.float64).copy()
    point = np.ascontiguousarray(prob["point"], np.float64).copy()
    keep = dict(pf=np.ascontiguousarray(prob["pose_fixed"], np.uint8),
                lf=None if prob.get("point_fixed") is None else np.ascontiguousarray(prob["point_fixed"], np.uint8),
                op=np.ascontiguousarray(prob["obs_pose"], np.int32), ol=np.ascontiguousarray(prob["obs_point"], np.int32),
                uv=np.ascontiguousarray(prob["obs_uv"], np.float64), info=np.ascontiguousarray(prob["obs_info"], np.float64),
                ei=np.ascontiguousarray(prob["edge_i"], np.int32), ej=np.ascontiguousarray(prob["edge_j"], np.int32),
                em=np.ascontiguousarray(prob["edge_meas"], np.float64), ew=np.ascontiguousarray(prob["edge_info"], np.float64))
    P = BaProblem(len(pose), len(point), len(keep["op"]), len(keep["ei"]), _p(pose, f64p), _p(keep["pf"], u8p), _p(point, f64p),
                  _p(keep["lf"], u8p), _p(keep["op"], i32p), _p(keep["ol"], i32p), _p(keep["uv"], f64p), _p(keep["info"], f64p),
                  float(prob["huber_delta"]), _p(keep["ei"], i32p), _p(keep["ej"], i32p), _p(keep["em"], f64p), _p(keep["ew"], f64p), max_iters)
    chi2 = np.zeros(max(len(keep["op"]), 1), np.float64)
    st = BaStats()
    rc = lib().mso_ba_solve(C.byref(P), _p(chi2, f64p), C.byref(st), int(bool(full_system)) | (int(bool(g2o_stale_chi2)) << 1) | ((int(force_reject) & 0xFF) << 8))
    assert rc == 0
    return dict(pose=pose, point=point, chi2=chi2[:len(keep["op"])],
                stats=dict(iters=st.iters, trials=st.trials_total, stop=st.stop_reason, lam=st.lambda_, chi2_init=st.chi2_init, chi2_final=st.chi2_final, min_abs_gain=st.min_abs_gain))


def se3_exp(u):
    u = np.ascontiguousarray(u, np.float64); out = np.zeros(7)
    lib().mso_se3_exp(_p(u, f64p), _p(out, f64p)); return out


def se3_log(p):
    p = np.ascontiguousarray(p, np.float64); out = np.zeros(6)
    lib().mso_se3_log(_p(p, f64p), _p(out, f64p)); return out


def se3_mul(a, b):
    a = np.ascontiguousarray(a, np.float64); b = np.ascontiguousarray(b, np.float64); out = np.zeros(7)
    lib().mso_se3_mul(_p(a, f64p), _p(b, f64p), _p(out, f64p)); return out


def ba_proj_edge(pose, X, uv):
    pose = np.ascontiguousarray(pose, np.float64); X = np.ascontiguousarray(X, np.float64); uv = np.ascontiguousarray(uv, np.float64)
    e, Jp, Jl = np.zeros(2), np.zeros((2, 6)), np.zeros((2, 3))
    lib().mso_ba_proj_edge(_p(pose, f64p), _p(X, f64p), _p(uv, f64p), _p(e, f64p), _p(Jp, f64p), _p(Jl, f64p))
    return e, Jp, Jl


def ba_pose_edge(Ti, Tj, M):
    Ti = np.ascontiguousarray(Ti, np.float64); Tj = np.ascontiguousarray(Tj, np.float64); M = np.ascontiguousarray(M, np.float64)
    e, Ji, Jj = np.zeros(6), np.zeros((6, 6)), np.zeros((6, 6))
    lib().mso_ba_pose_edge(_p(Ti, f64p), _p(Tj, f64p), _p(M, f64p), _p(e, f64p), _p(Ji, f64p), _p(Jj, f64p))
    return e, Ji, Jj
