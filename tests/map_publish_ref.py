"""ms_map_publish restated in numpy: the specification of the call (the header section of the same number).

publishMapForViewer (mapper_helpers.cpp:814-879) and updatePointCloudRecording (:881-909) on the map tables.  A table set is a dict:
    mp_pos [n_mp, 3] float64, mp_norm [n_mp, 3] float32, mp_flags [n_mp] uint8, mp_live [n_mp] uint8, n_obs [n_mp] int32,
    mp_color [n_mp, 3] uint8 or None, kf_mp [n_kf, stride] int32, kf_pose [n_kf, 12] float64
Row r is PRESENT iff 0 <= r < n_mp and mp_live[r] != 0; an entry is VALID iff 0 <= r < n_mp (as uint32); flags & 3: 3 TRIANGULATED, 2 UNSURE,
0 NOT_TRIANGULATED.  The record state is rec_pos [n_mp, 3] float32 and rec_state [n_mp] uint8 (0 never recorded, 1 recorded, 2 removed)."""
import numpy as np

VIEW, RECORD = 1, 2
NEW, MOVED, REMOVED = 1, 2, 3
OK, INVALID, CAPACITY = 0, -1, -4
F = np.float32
PUB = (("pub_row", np.int32, 1), ("pub_pos", F, 3), ("pub_norm", F, 3), ("pub_color", F, 3), ("pub_status", np.uint8, 1), ("pub_bits", np.uint8, 1))
EV = (("ev_row", np.int32, 1), ("ev_kind", np.uint8, 1), ("ev_pos", F, 3), ("ev_norm", F, 3))


def valid_rows(entries, n_mp):
    """the VALID entries of a list, as a boolean mark per row"""
    mark = np.zeros(n_mp, bool)
    e = np.asarray(entries, np.int32).reshape(-1).view(np.uint32)
    mark[e[e < n_mp].astype(np.int64)] = True
    return mark


def pose_wc(pose):
    """the rigid inverse of rows 0-2 of poseCW [12] as a row-major 4 x 4 float32 matrix: R^T | -R^T t in float64, the sum in the order
    -((R0j t0 + R1j t1) + R2j t2), then one cast"""
    P = np.asarray(pose, np.float64).reshape(12)
    out = np.zeros((4, 4), F)
    for j in range(3):
        out[j, 0], out[j, 1], out[j, 2] = F(P[j]), F(P[4 + j]), F(P[8 + j])
        out[j, 3] = F(-((P[j] * P[3] + P[4 + j] * P[7]) + P[8 + j] * P[11]))
    out[3, 3] = 1
    return out


def empty_record(n_mp):
    return np.zeros((n_mp, 3), F), np.zeros(n_mp, np.uint8)


def grow_record(rec_pos, rec_state, n_mp):
    """the caller's step when n_mp grows: zeros behind what is there"""
    p, s = empty_record(n_mp)
    p[:len(rec_pos)], s[:len(rec_state)] = rec_pos, rec_state
    return p, s


def map_publish(t, rec_pos, rec_state, what, current_slot=-1, min_record_obs=4, local_rows=(), kf_list=(), cap_pub=None, cap_ev=None):
    """Returns (rc, out, rec_pos, rec_state): out holds counts [8], pose_wc [n_list, 4, 4] and, on success, the PUB and EV arrays cut to
    n_pub / n_ev; the record state is the new one (the given arrays are not written; on a refusal they come back as they are)."""
    n_mp = len(t["mp_flags"])
    with np.errstate(over="ignore", invalid="ignore"):
        p = t["mp_pos"].astype(F)                            # cast<float>(): round to nearest even, overflow to inf
    present = t["mp_live"] != 0
    out = {}
    # ---- view (:823-839)
    published = present & ((t["mp_flags"] & 3) != 0) if what & VIEW else np.zeros(n_mp, bool)
    local = valid_rows(local_rows, n_mp)
    visible = valid_rows(t["kf_mp"][current_slot], n_mp) if current_slot >= 0 else np.zeros(n_mp, bool)
    rows = np.flatnonzero(published)
    color = np.zeros((n_mp, 3), F) if t.get("mp_color") is None else t["mp_color"].astype(F) / F(255.0)
    view = dict(pub_row=rows.astype(np.int32), pub_pos=p[rows], pub_norm=t["mp_norm"][rows], pub_color=color[rows].astype(F),
                pub_status=np.where(t["mp_flags"][rows] & 1, 0, 2).astype(np.uint8), pub_bits=(local[rows] | visible[rows].astype(np.uint8) << 1).astype(np.uint8))
    skipped = int((present & ~published).sum()) if what & VIEW else 0
    # ---- record (:881-909)
    kind = np.zeros(n_mp, np.uint8)
    if what & RECORD:
        enough = present & (t["n_obs"] >= min_record_obs)
        kind[enough & (rec_state != 1)] = NEW
        kind[enough & (rec_state == 1) & (rec_pos != p).any(axis=1)] = MOVED     # float comparison: -0 == 0, a NaN differs
        kind[~present & (rec_state == 1)] = REMOVED
    erows = np.flatnonzero(kind)
    gone = kind[erows] == REMOVED
    ev = dict(ev_row=erows.astype(np.int32), ev_kind=kind[erows], ev_pos=np.where(gone[:, None], F(0), p[erows]).astype(F),
              ev_norm=np.where(gone[:, None], F(0), t["mp_norm"][erows]).astype(F))
    out["counts"] = np.array([len(rows), len(erows), (kind == NEW).sum(), (kind == MOVED).sum(), (kind == REMOVED).sum(), local[rows].sum(), visible[rows].sum(), skipped], np.int32)
    out["pose_wc"] = np.array([pose_wc(t["kf_pose"][k]) for k in kf_list], F).reshape(len(kf_list), 4, 4)
    if (cap_pub is not None and len(rows) > cap_pub) or (cap_ev is not None and len(erows) > cap_ev):
        return CAPACITY, out, rec_pos, rec_state
    out.update(view)
    out.update(ev)
    if not what & RECORD:                                    # the record state is not read and may be None
        return OK, out, rec_pos, rec_state
    new_pos, new_state = rec_pos.copy(), rec_state.copy()
    moved = erows[~gone]
    new_pos[moved] = p[moved]
    new_state[moved] = 1
    new_state[erows[gone]] = 2
    return OK, out, new_pos, new_state
