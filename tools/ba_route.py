"""Which kernel ms_ba_solve launches for a batch of bundle-adjustment problems: the host's routing rule restated on the problem dicts of tests/ba_synth.py.
Shared by tools/ba_fuzz.py and tests/ba_scenes.py (plain numpy, no GPU)."""
import numpy as np


def route(probs, team):
    """The kernel ms_ba_solve launches for this batch (ba.hip: ms_ba_create's per-problem flags, ms_ba_solve's choice): k_ba_pose_only when every problem has
    ONE free pose, at most PO_MAXE = 8 SE3 edges touching it and every point fixed, and no team above 1 was asked for; k_ba_one_pose when every problem has
    ONE free pose, at least one free point, at most OP_NT = 512 SE3 edges and at most PO_MAXE touching the free pose; else k_ba_lm."""
    po = op = True
    for p in probs:
        free = np.flatnonzero(p["pose_fixed"] == 0)
        touching = int(((p["edge_i"] == free[0]) | (p["edge_j"] == free[0])).sum()) if len(free) == 1 else 0
        one = len(free) == 1 and touching <= 8
        all_fixed = (p.get("point_fixed") is not None and bool(np.all(p["point_fixed"] != 0))) or len(p["point"]) == 0
        po = po and one and all_fixed
        op = op and one and not all_fixed and len(p["edge_i"]) <= 512
    return "pose_only" if po and team <= 1 else "one_pose" if op else "general"
