"""The front end's per-frame chain on ONE set of map tables: the existing restatements composed, no rule restated here.

The state is one dict of numpy arrays under the names map_extract_ref uses for its destination (map_extract_ref.DST) plus what the
host keeps beside the device tables: kf_id [n_kf] (the slots' KfIds, -1 empty), desc_base [n_kf] (the slots' first descriptor in
desc_pool, -1 none), rec_pos / rec_state (the record of ms_map_publish), cams [n_kf, 6], focal [n_kf].  A step is a thin adapter:
it hands views of the state to the step's own restatement and writes the result back.

    step       restatement                                              writes back
    extract    map_extract_ref.extract                                  every DST array; kf_id, desc_base from the active list
    admit      frame_admit_ref.frame_admit                              frame_admit_ref.TABLES; kf_id[slot], desc_base[slot] = -1
    bind       match_tracked_ref.walk, .triangulate_tracked             match_tracked_ref.TABLES and the row fields
    refresh    match_tracked_ref.finish                                 the row fields (in place)
    pose       pose_tables_ref.gather / problem / apply                 kf_pose
    finish     frame_finish_ref.finish                                  frame_finish_ref.TABLES; kf_id[removed] = -1
    counts     map_cull_ref.observation_count                           n_obs
    publish    map_publish_ref.map_publish                              rec_pos, rec_state

The conversions (where two restatements want the same field in different shapes; each one is a place where two steps could disagree
unnoticed, none copies a value):
  C1  names.  map_extract_ref / frame_finish_ref / map_publish_ref: mp_pos, mp_norm, mp_min_dist, mp_max_dist, mp_desc, kp_x .. kp_depth,
      kf_pose, desc_pool.  match_tracked_ref: table{pos, norm, min_dist, max_dist, desc}, kp{x, y, octave, depth}, poses, pool.
      pose_tables_ref: mp_pos, poses, kp{...}, sigma, n_mp as a number.  The adapters pass VIEWS, so the in-place stages of
      match_tracked_ref (triangulate_tracked, finish) write the one state.
  C2  kf_id and desc_base are host arrays per DESTINATION slot.  The extract gives them by the active list (kf_id[i] =
      src.kf_id[active[i]], desc_base[i] = dst_desc_base[i], -1 behind); the admit sets kf_id[slot] (match_tracked_ref.observations
      and FIRST_LAST skip a slot whose kf_id is < 0, so it must be set BEFORE the match) and desc_base[slot] = -1; the finish sets
      kf_id = -1 for the removed slots.  No device call writes either.
  C3  "no map point".  frame_admit_ref and map_extract_ref write -1; frame_finish_ref writes -1; match_tracked_ref, pose_tables_ref,
      frame_finish_ref and map_cull_ref read "outside [0, n_mp)" as none, map_extract_ref and pose_tables_ref additionally "not live".
      On the destination tables the difference never shows: the extract drops entries of rows that are not live, the finish removes a
      row only when no remaining slot lists it (invariant I1), and no step writes an entry other than -1 or a live row.
  C4  the track of a keypoint.  frame_admit_ref refuses an id < 0 and hands kp_track = id down untouched; match_tracked_ref reads
      kp_track < 0 as "no track" (outcome 0) and indexes track_row[id - track_base] unchecked (the device refuses an id outside the
      window with MS_ERR_INVALID for the whole frame).  So behind ms_frame_admit outcome 0 cannot occur (keyframe.cpp:129 gives every
      kept feature its id), and the caller's window [track_base, track_base + n_track) has to cover every id the tracker hands over.
  C5  mp_flags is uint8 everywhere; bit 0 TRIANGULATED, bit 1 usable.  match_tracked_ref writes 0 / 2 / 3 (FLAG_OF_STATUS),
      frame_finish_ref and the extract's tail write 0; map_publish_ref reads `& 3`, the others `& 1`.
  C6  n_obs.  The extract writes the transpose count of the ACTIVE slots for every destination row, the finish rewrites it for the rows
      a removed slot lists, ms_observation_count for every row; the match and the admit do not write it.  check_n_obs() says where it
      is the transpose and names the stale rows elsewhere.
  C7  the solved pose.  pose_tables_ref.apply takes the solver's pose [7]; the CPU chain passes the oracle's, the GPU test the device's
      bytes, and every later step continues from kf_pose as apply() left it.
  C8  the record (rec_pos, rec_state) is indexed by DESTINATION row.  A second extract renumbers the rows, so across it the record
      compares a row with whatever point had that number before: deterministic, and the same on both sides of the comparison, but a
      caller that wants the reference's per-MpId record has to carry it over through row_src of the two copies.

The scene is a world model (build_world): 3-D points, a camera on a smooth path, keyframes and tracker frames whose features are the
points' projections with track ids.  The back end's keyframe chain (ms_keyframe_admit ... cull) can be added as further steps of
apply_step on the SOURCE tables in the same way; nothing of it is here."""
import numpy as np

import ba_synth
import ba_window_ref as W
import frame_admit_ref as FA
import frame_finish_ref as FF
import map_cull_ref as MC
import map_extract_ref as ME
import map_publish_ref as MP
import map_refresh_ref as MR
import match_tracked_ref as MT
import obs_lists_ref as OL
import pose_tables_ref as PT
import triangulate_ref as TR

F = np.float32
N_SRC_KF, STRIDE, N_SRC_MP, TRACK_BASE, N_TRACK, N_DST_KF = 10, 320, 1500, 1000, 2600, 8
CAM = (500.0, 500.0, 320.0, 240.0, 640, 480)
FOCAL = 500
SRC_SLOT = (7, 2, 9, 0, 5, 3, 8, 1, 6)                       # the slot of the keyframe at path index 0 .. 8; slot 4 is empty
EMPTY_SRC_SLOT = 4
N_FRAMES = 6
FRAME_SLOT = (5, 6, 7, 5, 6, 7)                              # frame 3 goes where frame 0 was, frame 4 where frame 1 was
FRAME_STAYS = (False, False, True, False, False, True)
OLDEST_DST_SLOT = 0                                          # the oldest active keyframe: removed after frame 2
MIN_RECORD_OBS = 4
SETTINGS = TR.settings(rel_reprojection_threshold=0.02)
VIEW_COS_LIMIT = 0.5
ROW_NAMES = dict(pos="mp_pos", norm="mp_norm", min_dist="mp_min_dist", max_dist="mp_max_dist", desc="mp_desc")
KP_NAMES = dict(x="kp_x", y="kp_y", octave="kp_octave", depth="kp_depth")


def kf_id_at(idx):
    return 10 + 3 * idx


def true_pose(idx):
    """(R, c) of the camera at path index idx: 0.1 a step along x, a slow sway."""
    R = TR.rotation(0.01 * np.sin(0.9 * idx), 0.012 * np.sin(0.6 * idx + 1.0), 0.008 * np.cos(0.8 * idx))
    return R, np.array([0.1 * idx, 0.02 * np.sin(0.7 * idx), 0.015 * np.cos(0.5 * idx)])


def pose12(R, c):
    return np.concatenate([R, (-R @ c)[:, None]], 1).reshape(12)


def project(idx, X):
    R, c = true_pose(idx)
    pc = R @ (X - c)
    return CAM[0] * pc[0] / pc[2] + CAM[2], CAM[1] * pc[1] / pc[2] + CAM[3], float(np.linalg.norm(pc)), pc[2]


def inside(u, v, z, margin=8.0):
    return z > 0.5 and margin <= u < CAM[4] - margin and margin <= v < CAM[5] - margin


# ------------------------------------------------------------------------------------------------------------------------------ world
def build_world(seed=5):
    """The source tables, the changed source of the second copy, the frames and the rasters.  See the module docstring of
    tests/test_frame_chain_ref.py for what the scene has to contain; that file asserts it."""
    rng = np.random.default_rng(seed)
    n_mp = N_SRC_MP
    # ---- points: visible from path index first .. first + length - 1
    first = rng.integers(-2, 14, n_mp)
    length = rng.choice([1, 2, 3, 5, 6, 8, 11], n_mp, p=[0.15, 0.15, 0.15, 0.2, 0.15, 0.1, 0.1])
    X = np.zeros((n_mp, 3))
    for r in range(n_mp):
        Rm, cm = true_pose(first[r] + 0.5 * (length[r] - 1))
        zc = rng.uniform(3.0, 10.0)
        X[r] = Rm.T @ np.array([rng.uniform(-0.4, 0.4) * zc, rng.uniform(-0.33, 0.33) * zc, zc]) + cm
    covers = lambda r, idx: first[r] <= idx < first[r] + length[r]

    def keyframe_rows(idx, cap=300):
        rows = [r for r in rng.permutation(n_mp) if covers(r, idx) and inside(*[project(idx, X[r])[i] for i in (0, 1, 3)])]
        return rows[:cap]

    kf_mp = np.full((N_SRC_KF, STRIDE), -1, np.int32)
    kp = dict(kp_x=rng.uniform(0, 640, (N_SRC_KF, STRIDE)).astype(F), kp_y=rng.uniform(0, 480, (N_SRC_KF, STRIDE)).astype(F),
              kp_octave=rng.integers(0, 8, (N_SRC_KF, STRIDE)).astype(np.int32), kp_depth=np.full((N_SRC_KF, STRIDE), -1, F))
    kf_id, n_kp = np.full(N_SRC_KF, -1, np.int32), np.zeros(N_SRC_KF, np.int32)
    kf_pose = rng.uniform(-2, 2, (N_SRC_KF, 12))

    def put_keyframe(slot, idx, cap=300):
        rows = keyframe_rows(idx, cap)
        js = rng.permutation(len(rows) + 12)[:len(rows)]     # a dozen keypoints stay unbound
        for r, j in zip(rows, js):
            u, v, rng_depth, _ = project(idx, X[r])
            kf_mp[slot, j] = r
            kp["kp_x"][slot, j], kp["kp_y"][slot, j] = u + rng.normal(0, 0.3), v + rng.normal(0, 0.3)
            if rng.random() < 0.2:
                kp["kp_depth"][slot, j] = rng_depth * (1.0 + rng.normal(0, 1e-3))
        kf_id[slot], n_kp[slot] = kf_id_at(idx), len(rows) + 12
        kf_pose[slot] = pose12(*true_pose(idx))

    for idx, slot in enumerate(SRC_SLOT):
        put_keyframe(slot, idx)
    # ---- rows
    n_seen = np.bincount(kf_mp[kf_mp >= 0], minlength=n_mp)
    flags = np.zeros(n_mp, np.uint8)
    u = rng.random(n_mp)
    flags[(n_seen >= 3) & (u < 0.65)] = 3
    flags[(n_seen >= 3) & (u >= 0.65) & (u < 0.75)] = 2
    flags[(n_seen == 2) & (u < 0.45)] = 3
    flags[(n_seen == 2) & (u >= 0.45) & (u < 0.7)] = 2
    flags[(n_seen == 1) & (u < 0.3)] = 3
    noise = np.where(flags == 3, 0.004, np.where(flags == 2, 0.02, 0.3))
    mp_pos = X + rng.normal(0, 1, (n_mp, 3)) * noise[:, None]
    mp_norm, min_dist, max_dist = np.zeros((n_mp, 3), F), np.zeros(n_mp, F), np.zeros(n_mp, F)
    for r in range(n_mp):
        _, cm = true_pose(first[r] + 0.5 * (length[r] - 1))
        d = np.linalg.norm(cm - X[r])
        mp_norm[r] = ((cm - X[r]) / d + rng.normal(0, 0.03, 3)).astype(F)
        min_dist[r], max_dist[r] = d / 3.0, d * 1.5
    tri = np.flatnonzero(flags == 3)
    odd = rng.permutation(tri)[:len(tri) // 8]
    mp_norm[odd[::2]] = -mp_norm[odd[::2]]                   # turned away
    max_dist[odd[1::2]] = min_dist[odd[1::2]] * F(1.01)      # beyond maxViewingDistance
    mp_live = np.ones(n_mp, np.uint8)
    mp_live[rng.permutation(n_mp)[:60]] = 0                  # dead rows, still listed and still carrying their track
    ids = iter((TRACK_BASE + rng.permutation(N_TRACK)).tolist())
    mp_track, track_row = np.full(n_mp, -1, np.int32), np.full(N_TRACK, -1, np.int32)
    for r in range(n_mp):
        if rng.random() < 0.88:
            mp_track[r] = next(ids)
            track_row[mp_track[r] - TRACK_BASE] = r
    old_track = {}
    for r in rng.permutation(np.flatnonzero(mp_track >= 0))[:40]:      # recycled: the old track still names the row
        old_track[int(r)] = int(mp_track[r])
        mp_track[r] = next(ids)
        track_row[mp_track[r] - TRACK_BASE] = r
    nowhere = [next(ids) for _ in range(4)]                  # tracks whose entry lies outside the table
    track_row[np.array(nowhere) - TRACK_BASE] = [n_mp, n_mp + 7, -2 ** 31, -2]
    fresh = [next(ids) for _ in range(400)]                  # tracks without a map point
    # ---- stale and invalid entries
    kf_mp[EMPTY_SRC_SLOT, :9] = [3, 700, n_mp, -5, 41, 41, 1499, -1, 2 ** 30]
    for slot in SRC_SLOT:
        free = np.flatnonzero(kf_mp[slot] == -1)
        kf_mp[slot, free[-1]], kf_mp[slot, free[-2]] = n_mp + 3, -7
    # ---- descriptors
    desc_base = np.full(N_SRC_KF, -1, np.int32)
    at = 5
    for slot in rng.permutation(N_SRC_KF):
        if kf_id[slot] >= 0 and slot != SRC_SLOT[6]:         # one active keyframe has no descriptors
            desc_base[slot] = at
            at += n_kp[slot] + 3
    src = dict(kf_mp=kf_mp, kf_id=kf_id, mp_flags=flags, mp_live=mp_live, mp_pos=mp_pos, mp_norm=mp_norm, mp_min_dist=min_dist, mp_max_dist=max_dist,
               mp_desc=rng.integers(0, 2 ** 32, (n_mp, 8), dtype=np.uint32), mp_track=mp_track, kf_pose=kf_pose, track_row=track_row, track_base=TRACK_BASE,
               desc_pool=rng.integers(0, 2 ** 32, (at + 400, 8), dtype=np.uint32), desc_base=desc_base, n_kp=n_kp, **kp)
    active1 = [SRC_SLOT[i] for i in range(4, 9)]             # ascending KfId
    # ---- the changed source of the second copy: a keyframe at frame 2's place in the empty slot, rows moved, rows culled
    src2 = {k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in src.items()}
    kf_mp, kf_id, n_kp, kf_pose = src2["kf_mp"], src2["kf_id"], src2["n_kp"], src2["kf_pose"]
    kp = {k: src2[k] for k in KP_NAMES.values()}
    kf_mp[EMPTY_SRC_SLOT] = -1
    put_keyframe(EMPTY_SRC_SLOT, 11, 120)
    src2["desc_base"][EMPTY_SRC_SLOT] = at
    listed = np.unique(kf_mp[active1][(kf_mp[active1] >= 0) & (kf_mp[active1] < n_mp)])
    moved = rng.permutation(listed)[:25]
    src2["mp_pos"][moved] += rng.normal(0, 0.01, (25, 3))
    src2["mp_live"][rng.permutation(listed)[:len(listed) // 4]] = 0
    active2 = active1 + [EMPTY_SRC_SLOT]
    # ---- the oldest active keyframe's own rows: frame 3 still tracks a few of them
    others = src["kf_mp"][[s for s in SRC_SLOT[5:9]]]
    own = [int(r) for r in src["kf_mp"][active1[0]] if 0 <= r < n_mp and src["mp_live"][r] and src["mp_track"][r] >= 0 and not (others == r).any()]
    # ---- rasters
    image = np.where(rng.random((480, 640)) < 0.2, rng.uniform(2, 9, (480, 640)), -1.0).astype(F)
    mask = np.ones((480, 640), np.uint8)
    # ---- frames
    frames = []
    for f in range(N_FRAMES):
        idx = 9 + f
        feats = []                                           # (track id, x, y, depth)
        rows = [r for r in rng.permutation(n_mp) if covers(r, idx) and mp_track[r] >= 0 and inside(*[project(idx, X[r])[i] for i in (0, 1, 3)])]
        off = set(int(r) for r in rng.permutation([r for r in rows if flags[r] == 3])[:14])
        for r in rows[:255]:
            u, v, rng_depth, _ = project(idx, X[r])
            t = old_track[r] if r in old_track and rng.random() < 0.5 else int(mp_track[r])
            feats.append((t, u + rng.normal(0, 0.2), v + rng.normal(0, 0.2) + (40.0 if r in off and v < 400 else 0.0),
                          rng_depth * (1.0 + rng.normal(0, 1e-3)) if rng.random() < 0.2 else -1.0))
        if f == 3:                                           # the tracker still follows a few points that only the removed keyframe saw
            have = {t for t, _, _, _ in feats}
            for r in [r for r in own if first[r] + length[r] <= 9 and int(mp_track[r]) not in have][:4]:
                u, v, _, _ = project(idx, X[r])
                feats.append((int(mp_track[r]), min(max(u, 20.0), 620.0), min(max(v, 20.0), 460.0), -1.0))
        for t in fresh[40 * f:40 * f + 36] + nowhere:
            feats.append((t, rng.uniform(20, 620), rng.uniform(20, 460), -1.0 if rng.random() < 0.7 else rng.uniform(2, 8)))
        order = rng.permutation(len(feats))
        feats = [feats[i] for i in order]
        n = len(feats)
        feat = dict(id=np.array([t for t, _, _, _ in feats], np.int32), x=np.array([x for _, x, _, _ in feats], F), y=np.array([y for _, _, y, _ in feats], F),
                    depth=np.array([d for _, _, _, d in feats], F), keep=np.ones(n, np.uint8))
        drop = rng.permutation(n)[:14]
        feat["keep"][drop[:7]] = 0
        for i in drop[7:]:
            mask[int(FA.rint_i32(feat["y"][i:i + 1])[0]), int(FA.rint_i32(feat["x"][i:i + 1])[0])] = 0
        R, c = true_pose(idx)
        Rp = ba_synth._rotvec(rng.normal(0, 0.002, 3)) @ R
        pose = np.concatenate([Rp, (-R @ c + rng.normal(0, 0.004, 3))[:, None]], 1).reshape(12)
        frames.append(dict(feat=feat, slot=FRAME_SLOT[f], pose=pose, kf_id=kf_id_at(idx), idx=idx, stays=FRAME_STAYS[f]))
    # the previous keyframe of each frame: (destination slot, path index)
    prev = [(4, 8), (4, 8), (4, 8), (FRAME_SLOT[2], 11), (5, 11), (5, 11)]
    for f, fr in enumerate(frames):
        fr["prev_slot"] = prev[f][0]
        Rf, cf = true_pose(fr["idx"])
        Rq, cq = true_pose(prev[f][1])
        true = [ba_synth._pose(R, -R @ c) for R, c in ((Rf, cf), (Rq, cq))]
        M = ba_synth._compose(ba_synth._pose(ba_synth._rotvec(rng.normal(0, 0.001, 3)), rng.normal(0, 0.002, 3)), ba_synth._compose(true[1], ba_synth._inverse(true[0])))
        fr["edge_meas"], fr["edge_info"] = M, (np.diag([100.0 ** 2] * 3 + [50.0 ** 2] * 3) * (0.26667 / 0.1)).reshape(36)
    n_rows1 = int(ME.extract(src, active1, ME.sizes(src, N_DST_KF, n_mp, len(src["desc_pool"])))["counts"][0])
    pool_dst = int(max(sum(s["n_kp"][a] for a in act if s["desc_base"][a] >= 0) for s, act in ((src, active1), (src2, active2)))) + 8
    return dict(src=src, src2=src2, active1=active1, active2=active2, frames=frames, image=image, mask=mask, n_mp_dst=n_rows1 + 40, pool_dst=pool_dst,
                own_rows_of_oldest=own, local_rows=np.unique(src["kf_mp"][active1[2:]][src["kf_mp"][active1[2:]] >= 0])[:200].astype(np.int32))


_WORLD = {}


def world(seed=5):
    """build_world(seed), computed once and shared; not to be changed."""
    if seed not in _WORLD:
        _WORLD[seed] = build_world(seed)
    return _WORLD[seed]


def schedule():
    """The steps in order: (name, argument)."""
    steps = [("extract", 1), ("counts", None), ("publish", 4)]
    for f in range(N_FRAMES):
        steps += [("admit", f), ("bind", f), ("refresh", f), ("pose", f), ("finish", f)]
        if f == 2:
            steps += [("remove", [OLDEST_DST_SLOT]), ("counts", None), ("publish", FRAME_SLOT[2])]
        if f == 3:
            steps += [("source_change", None), ("extract", 2)]
        if f == 5:
            steps += [("counts", None), ("publish", FRAME_SLOT[5])]
    return steps


# ------------------------------------------------------------------------------------------------------------------------------ state
def sizes(w, src):
    return ME.sizes(src, N_DST_KF, w["n_mp_dst"], w["pool_dst"])


def initial_state(w, fill=0):
    """The destination tables before the first extract (a byte pattern) and the host's arrays."""
    z = sizes(w, w["src"])
    st = ME.fresh_dst(w["src"], z, fill)
    rec_pos, rec_state = MP.empty_record(z["n_mp_dst"])
    st.update(kf_id=np.full(N_DST_KF, -1, np.int32), desc_base=np.full(N_DST_KF, -1, np.int32), rec_pos=rec_pos, rec_state=rec_state,
              cams=np.tile(np.array(CAM, np.float64), (N_DST_KF, 1)), focal=np.full(N_DST_KF, FOCAL, np.int32), track_base=TRACK_BASE, n_mp=z["n_mp_dst"])
    return st


def device_names(st):
    """The arrays of the state that live on the device."""
    return [k for k in ME.DST if k in st] + ["rec_pos", "rec_state"]


def match_state(st):
    """C1: the state as match_tracked_ref reads and (in place) writes it."""
    return dict(kf_mp=st["kf_mp"], kf_id=st["kf_id"], poses=st["kf_pose"], cams=st["cams"], focal=st["focal"], kp={k: st[v] for k, v in KP_NAMES.items()},
                desc_base=st["desc_base"], pool=st["desc_pool"], table={k: st[v] for k, v in ROW_NAMES.items()}, mp_flags=st["mp_flags"], mp_live=st["mp_live"],
                mp_track=st["mp_track"], track_row=st["track_row"], track_base=st["track_base"], S=SETTINGS, sf=MR.scale_factors(), view_cos_limit=VIEW_COS_LIMIT)


def pose_scene(st):
    """C1: the state as pose_tables_ref reads it."""
    return dict(n_mp=st["n_mp"], kf_mp=st["kf_mp"], mp_flags=st["mp_flags"], mp_live=st["mp_live"], mp_pos=st["mp_pos"], poses=st["kf_pose"],
                kp={k: st[v] for k, v in KP_NAMES.items()}, sigma=W.sigma_levels())


def pose_frame(fr, n_kp):
    return dict(slot=fr["slot"], prev_slot=fr["prev_slot"], n_kp=n_kp, cam=CAM, focal=FOCAL, edge_meas=fr["edge_meas"], edge_info=fr["edge_info"],
                min_visible=PT.MIN_VISIBLE, max_iters=PT.MAX_ITERS, huber_delta=ba_synth.HUBER_DELTA)


def listed_rows(st, slots):
    """The rows the slots list (valid entries, each once)."""
    e = np.asarray(st["kf_mp"], np.int64)[list(slots)].reshape(-1)
    return np.unique(e[(e >= 0) & (e < st["n_mp"])])


def apply_step(st, w, step, run, solve=None):
    """One step of schedule() on the state in place.  run: a dict carried through the schedule (the current source, per frame the
    admit's and the match's outputs).  solve(prob, frame, g) -> the solver's pose [7] (the pose step only).  Returns the step's host outputs."""
    name, arg = step
    if name == "source_change":
        run["src"] = w["src2"]
        return {}
    if name == "extract":
        src, active = run.setdefault("src", w["src"]), w["active%d" % arg]
        z = sizes(w, src)
        out = ME.extract(src, active, z, {k: st[k] for k in ME.dst_names(src)})
        assert out["rc"] == ME.OK, out["counts"]
        for k in ME.dst_names(src):
            st[k] = out[k]
        st["kf_id"][:], st["desc_base"][:] = -1, -1           # C2
        st["kf_id"][:len(active)], st["desc_base"][:len(active)] = src["kf_id"][active], out["dst_desc_base"]
        return dict(counts=out["counts"], dst_desc_base=out["dst_desc_base"])
    if name == "counts":
        n_obs, first, last = MC.observation_count(st["kf_mp"], st["n_mp"], st["kf_id"])
        st["n_obs"] = n_obs
        return {}
    if name == "publish":
        kf_list = [s for s in range(N_DST_KF) if st["kf_id"][s] >= 0]
        rc, out, st["rec_pos"], st["rec_state"] = MP.map_publish(st, st["rec_pos"], st["rec_state"], MP.VIEW | MP.RECORD, arg, MIN_RECORD_OBS, w["local_rows"], kf_list)
        assert rc == MP.OK
        return dict(out, kf_list=kf_list)
    if name == "remove":
        listed = listed_rows(st, arg)
        out = FF.finish({k: st[k] for k in ("kf_mp", "kf_id", "mp_flags", "mp_live", "mp_pos", "mp_track", "n_obs")}, arg, -1, 0)
        assert out["rc"] == FF.OK
        for k in FF.TABLES:
            st[k] = out[k]
        st["kf_id"][arg] = -1                                # C2
        return dict({k: out[k] for k in ("cloud_row", "cloud_kp", "cloud_track", "cloud_pos", "removed_rows", "counts")}, listed_rows=listed)
    fr = w["frames"][arg]
    fx = run.setdefault(("frame", arg), {})
    if name == "admit":
        rc, T, out = FA.frame_admit({k: st[k] for k in FA.TABLES}, st["n_mp"], fr["feat"], fr["slot"], fr["pose"], w["image"], w["mask"])
        assert rc == FA.OK, (arg, rc)
        st.update(T)
        st["kf_id"][fr["slot"]], st["desc_base"][fr["slot"]] = fr["kf_id"], -1      # C2
        fx["admit"] = out
        return out
    if name == "bind":
        walked = MT.walk(match_state(st), dict(slot=fr["slot"], kp_track=fx["admit"]["kp_track"]), np.zeros(0, np.int32))
        assert walked["rc"] == 0, walked["violations"]
        for k in MT.TABLES:
            st[k] = walked["state"][k]
        for k, v in ROW_NAMES.items():
            st[v] = walked["state"]["table"][k]
        walked["status"] = MT.triangulate_tracked(match_state(st), walked["tracked_rows"])
        fx["match"] = walked
        return {k: walked[k] for k in ("outcome", "counts", "created_rows", "created_kp", "tracked_rows", "checked_rows", "status")}
    if name == "refresh":
        m = fx["match"]
        m["refresh_rows"] = MT.finish(match_state(st), m["tracked_rows"], m["checked_rows"], m["has_desc"])
        return dict(refresh_rows=m["refresh_rows"])
    if name == "pose":
        frame = pose_frame(fr, len(fx["admit"]["kp_track"]))
        g = PT.gather(pose_scene(st), frame)
        prob = PT.problem(frame, g)
        pose = np.asarray(solve(prob, frame, g), np.float64) if g["n"] >= frame["min_visible"] else g["pose"][0]
        poses, ran = PT.apply(st["kf_pose"], frame, g, pose, bool(np.isfinite(pose).all()))
        st["kf_pose"] = poses
        fx["pose"] = dict(g=g, prob=prob, frame=frame, ran=ran, pose=pose)
        return fx["pose"]
    if name == "finish":
        remove = [] if fr["stays"] else [fr["slot"]]
        listed = listed_rows(st, remove)
        out = FF.finish({k: st[k] for k in ("kf_mp", "kf_id", "mp_flags", "mp_live", "mp_pos", "mp_track", "n_obs")}, remove, fr["slot"], len(fx["admit"]["kp_track"]))
        assert out["rc"] == FF.OK
        for k in FF.TABLES:
            st[k] = out[k]
        st["kf_id"][remove] = -1                             # C2
        fx["finish"] = out
        return dict({k: out[k] for k in ("cloud_row", "cloud_kp", "cloud_track", "cloud_pos", "removed_rows", "counts")}, listed_rows=listed, remove=remove)
    raise ValueError(name)


# ------------------------------------------------------------------------------------------------------------------------------ invariants
def transposed_n_obs(st):
    start, _, _ = OL.transpose(st["kf_mp"], st["n_mp"], st["kf_id"])
    return np.diff(start).astype(np.int32)


def check_invariants(st, label=""):
    """I1 - I5 on a state (the restated one or a downloaded one with the host's kf_id beside it)."""
    n_mp, kf = st["n_mp"], np.asarray(st["kf_mp"], np.int64)
    for s in range(len(kf)):
        if st["kf_id"][s] < 0:
            continue
        e = kf[s][(kf[s] >= 0) & (kf[s] < n_mp)]
        assert (st["mp_live"][e] != 0).all(), (label, "I1", s, e[st["mp_live"][e] == 0][:5])
        assert len(np.unique(e)) == len(e), (label, "I2", s)
    tr = np.asarray(st["track_row"], np.int64)
    ok = (tr >= 0) & (tr < n_mp)
    ok[ok] = (st["mp_live"][tr[ok]] != 0) & (st["mp_track"][tr[ok]] == st["track_base"] + np.flatnonzero(ok))
    assert len(np.unique(tr[ok])) == int(ok.sum()), (label, "I3")
    tri = (st["mp_flags"] & 1) != 0
    assert np.isfinite(st["mp_pos"][tri]).all(), (label, "I4")
    empty = kf[np.asarray(st["kf_id"]) < 0]                  # I5: an empty slot of the destination can be admitted into
    assert not ((empty >= 0) & (empty < n_mp)).any(), (label, "I5")


def stale_n_obs(st):
    """The rows whose n_obs is not the transpose of kf_mp."""
    return np.flatnonzero(st["n_obs"] != transposed_n_obs(st))


def check_n_obs(st, step, out, label=""):
    """n_obs is the transpose exactly where the chain promises it: for every row after an extract and after ms_observation_count, for
    the rows a removed slot listed after a finish.  Returns the stale rows (to be recorded, not asserted) for every other step."""
    name = step[0]
    stale = stale_n_obs(st)
    if name in ("extract", "counts"):
        assert len(stale) == 0, (label, name, stale[:8])
    elif name in ("finish", "remove"):
        listed = out.get("listed_rows")
        if listed is not None:
            assert not np.isin(stale, listed).any(), (label, name, np.intersect1d(stale, listed)[:8])
    return stale
