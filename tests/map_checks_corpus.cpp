// map_checks_corpus -- one line per call of the 22 host-only ms_*_check twins of the map entry points: function, case, return code, message
// (tab separated).  tests/test_map_checks_corpus.py compares the output byte for byte with tests/golden/map_checks_corpus.txt, once linked
// against libmi355slam.so and once compiled together with csrc/map_checks.cpp alone under ASan and UBSan.  Public header only.
//
// Base shapes: 5 slots of stride 8, 10 map points, 3 levels, 3 candidates / queries / listed slots.  Every function gets an accepted call, the
// call with every size zero, a negative size, stride 0, a missing array, each cap it tests exceeded by one, and its last rejecting statement.
// The checks read HOST arguments only: small host arrays stand in for the device arrays, whose contents are never read.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "mi355slam.h"

namespace {

constexpr int kBig = MS_COVIS_MAX_KF + 1;                    // the longest host array a check may read: kf_id / kf_t at the slot cap plus one
int32_t kf_mp[40], kf_id[kBig], n_obs_tab[10], mp_track[10], track_row[6], kp_octave[40], kf_desc_base[5], kf_focal[5] = {500, 500, 500, 500, 500};
uint8_t mp_flags[10], mp_live[10];
double mp_pos[30], kf_pose[60], kf_t[kBig];
float mp_norm[30], mp_min_dist[10], mp_max_dist[10], kp_x[40], kp_y[40], kp_depth[40], scale_factors[3] = {1.f, 1.2f, 1.44f}, sigma[3] = {1.f, 1.44f, 2.0736f};
alignas(16) uint32_t mp_desc[80], desc_pool[320], q_desc[64], t_desc[64];
ms_pinhole cams[5];
// stand-ins for outputs and for device lists
int32_t out_i[64], zeros_i[MS_COVIS_MAX_QUERIES + 1];
uint8_t out_b[64], *no_masks[MS_COVIS_MAX_QUERIES + 1];
double out_d[64];
float out_f[64];
uint16_t out_h[64];

ms_obs_lists all_lists() { return ms_obs_lists{out_i, out_i, out_i, out_i, out_b, out_i, out_i, out_i, out_i, out_f, out_f, out_f}; }

template <class A, class F> void one(const char *name, F change) {
    A a;
    change(a);
    char why[512];
    std::memset(why, 0, sizeof(why));
    const int rc = a.call(why, sizeof(why));
    std::printf("%s\t%s\t%d\t%s\n", A::fn, name, rc, why);
}
#define CASE(A, name, ...) one<A>(name, [&](A &a) { (void)a; __VA_ARGS__; })
// the three caps of the keyframe table, each exceeded by one
#define TABLE_CAPS(A) CASE(A, "cap slots", a.n_kf = MS_COVIS_MAX_KF + 1); CASE(A, "cap map points", a.n_mp = MS_COVIS_MAX_MP)
#define STRIDE_CAP(A) CASE(A, "cap stride", a.stride = MS_COVIS_MAX_STRIDE + 1)

struct Refresh {
    static constexpr const char *fn = "ms_map_refresh_check";
    const double *pos = mp_pos, *pose = kf_pose;
    const float *norm = mp_norm, *scale = scale_factors;
    const uint32_t *desc = mp_desc, *pool = desc_pool;
    int n_mp = 10, n_kf = 5, n_pool = 40, n_rows = 3, n_levels = 3;
    int32_t rows[3] = {1, 4, 7}, obs_start[4] = {0, 2, 3, 5}, obs_kf[5] = {0, 1, 2, 3, 4}, obs_desc[5] = {0, 8, 16, 24, 32}, first_octave[3] = {0, 1, 2};
    const int32_t *p_rows = rows;
    int call(char *why, size_t n) {
        return ms_map_refresh_check(pos, norm, mp_min_dist, mp_max_dist, desc, n_mp, pose, n_kf, pool, n_pool, p_rows, n_rows, obs_start, obs_kf, obs_desc, first_octave, scale,
                                    n_levels, why, n);
    }
};

struct LoopCorrect {
    static constexpr const char *fn = "ms_loop_correct_check";
    int n_kf = 5, n_mp = 10, n_corr = 3, n_pts = 3;
    double T[8] = {1, 0, 0, 0, 0, 0, 0, 1}, lambda[3] = {0.5, 0.0, 1.0};
    int32_t slot[3] = {1, 3, 0}, row[3] = {2, 5, 9}, ref[3] = {0, 1, 2};
    uint8_t rigid[3] = {0, 1, 0};
    const int32_t *p_slot = slot;
    int call(char *why, size_t n) { return ms_loop_correct_check(kf_pose, n_kf, mp_pos, n_mp, T, p_slot, rigid, lambda, n_corr, row, ref, n_pts, why, n); }
};

struct Covis {
    static constexpr const char *fn = "ms_covisibility_check";
    int n_kf = 5, stride = 8, n_mp = 10, n_q = 3;
    const uint8_t *flags = mp_flags;
    ms_covis_query q[3] = {{1, -1, -1, 15, 0}, {3, 0, -1, 15, 1}, {0, -1, 4, 1, 0}};
    const ms_covis_query *p_q = q;
    int call(char *why, size_t n) { return ms_covisibility_check(kf_mp, n_kf, stride, flags, n_mp, p_q, n_q, out_i, out_i, why, n); }
};

struct Union {
    static constexpr const char *fn = "ms_map_point_union_check";
    int n_kf = 5, stride = 8, n_mp = 10, n_list = 3, n_u = 3;
    const uint8_t *flags = mp_flags;
    int32_t list[3] = {1, 3, 0};
    ms_union_problem u[3] = {{0, 2, -1, 0}, {2, 1, 1, 1}, {0, 0, -1, 0}};
    const ms_union_problem *p_u = u;
    int call(char *why, size_t n) { return ms_map_point_union_check(kf_mp, n_kf, stride, flags, n_mp, list, n_list, p_u, n_u, out_i, out_i, why, n); }
};

struct Cull {
    static constexpr const char *fn = "ms_map_cull_check";
    int n_kf = 5, stride = 8, n_mp = 10, n_cand = 3;
    const double *t = kf_t;
    int32_t cand[3] = {3, 0, 4};
    uint8_t keep[3] = {0, 1, 0};
    ms_cull_settings s = {1, 1, 2.0, 3, 0.9, 0};
    int call(char *why, size_t n) {
        return ms_map_cull_check(kf_mp, n_kf, stride, mp_flags, mp_live, n_mp, kf_id, t, cand, keep, n_cand, &s, out_i, out_b, out_i, out_i, why, n);
    }
};

struct Tri {
    static constexpr const char *fn = "ms_triangulate_check";
    int n_mp = 10, n_kf = 5, n_rows = 3, mode = MS_TRI_TME;
    int32_t rows[3] = {1, 4, 7}, obs_start[4] = {0, 2, 3, 5}, obs_kf[5] = {0, 1, 2, 3, 4}, obs_octave[5] = {0, 1, 2, 0, 1};
    const int32_t *p_rows = rows;
    ms_tri_settings s = {sigma, 3, 1.0, 2.0, 2.5f, 0};
    int call(char *why, size_t n) {
        return ms_triangulate_check(mp_pos, n_mp, kf_pose, n_kf, cams, kf_focal, p_rows, out_b, n_rows, obs_start, obs_kf, out_f, out_f, obs_octave, &s, mode, why, n);
    }
};

struct ObsLists {
    static constexpr const char *fn = "ms_observation_lists_check";
    int n_kf = 5, stride = 8, n_mp = 10, n_levels = 3, cap_rows = 8, cap_obs = 16;
    const uint8_t *flags = mp_flags;
    ms_obs_select sel = {MS_OBS_FROM_ROWS, MS_OBS_ALL, 1, 0, out_i, 3};
    const ms_obs_select *p_sel = &sel;
    ms_obs_lists out = all_lists();
    int call(char *why, size_t n) {
        return ms_observation_lists_check(kf_mp, n_kf, stride, n_mp, kf_id, flags, kp_x, kp_y, kp_octave, kp_depth, kf_desc_base, p_sel, n_levels, &out, cap_rows, cap_obs,
                                          out_i, out_i, why, n);
    }
};

struct Tracked {
    static constexpr const char *fn = "ms_match_tracked_check";
    int n_kf = 5, stride = 8, n_mp = 10, n_pool = 40, n_track = 6, n_kp = 6, n_new = 4;
    int32_t kp_track[6] = {100, -1, 103, 105, -1, 101}, new_rows[4] = {2, 5, 8, 9};
    ms_tracked_frame f = {1, {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}, {500.0, 510.0, 320.0, 240.0, 640, 480}, 500, 8, 100, sigma, 3, 2.5f, 0.5f};
    const ms_tracked_frame *p_f = &f;
    int call(char *why, size_t n) {
        return ms_match_tracked_check(kf_mp, n_kf, stride, mp_flags, mp_live, mp_pos, mp_norm, mp_min_dist, mp_max_dist, mp_desc, mp_track, n_mp, kp_x, kp_y, kp_octave,
                                      desc_pool, n_pool, track_row, n_track, p_f, kp_track, n_kp, new_rows, n_new, out_b, out_i, why, n);
    }
};

struct Finish {
    static constexpr const char *fn = "ms_match_tracked_finish_check";
    int n_rows = 3, n_mp = 10, n_checked = 2, append = 1, cap_refresh = 8;
    ms_obs_lists lists = all_lists();
    const uint32_t *desc = mp_desc;
    const int32_t *n_refresh = out_i;
    int32_t checked[2] = {1, 2};
    int call(char *why, size_t n) {
        return ms_match_tracked_finish_check(&lists, n_rows, mp_flags, desc_pool, desc, n_mp, checked, n_checked, append, out_i, cap_refresh, n_refresh, why, n);
    }
};

struct Fuse {
    static constexpr const char *fn = "ms_map_fuse_check";
    int n_kf = 5, stride = 8, n_mp = 10, n_track = 6, n_entries = 8, n_views = 3, max_dist = 50, source_slot = 2;
    int32_t mp_index[8] = {0, 1, 2, 3, 4, 5, 6, 7}, n_kept[3] = {2, 0, 3};
    ms_fuse_view views[3] = {{1, 0, 3}, {3, 3, 2}, {0, 5, 3}};
    const int32_t *counts = out_i;
    int call(char *why, size_t n) {
        return ms_map_fuse_check(kf_mp, n_kf, stride, mp_flags, mp_live, n_obs_tab, n_mp, mp_track, track_row, 100, n_track, out_i, out_i, out_h, mp_index, n_entries, views,
                                 n_kept, n_views, max_dist, source_slot, out_i, counts, out_i, why, n);
    }
};

struct Pairs {
    static constexpr const char *fn = "ms_map_replace_pairs_check";
    int n_kf = 5, stride = 8, n_mp = 10, n_track = 6, n_pairs = 3;
    int32_t pairs[6] = {1, 2, 3, 3, 2, 5};
    const int32_t *p_pairs = pairs;
    int call(char *why, size_t n) {
        return ms_map_replace_pairs_check(kf_mp, n_kf, stride, mp_flags, mp_live, n_obs_tab, n_mp, mp_track, track_row, 100, n_track, p_pairs, n_pairs, out_b, out_i, why, n);
    }
};

struct CreateLists {
    static constexpr const char *fn = "ms_create_points_lists_check";
    int n_kf = 5, stride = 8, n_mp = 10, cur = 1, adj = 3, n_kp1 = 6, n_kp2 = 8, n_new = 3, n_levels = 3, cap_rows = 8, cap_obs = 16;
    int32_t new_rows[3] = {2, 5, 8};
    const int32_t *matched = out_i;
    ms_obs_lists lists = all_lists();
    int call(char *why, size_t n) {
        return ms_create_points_lists_check(kf_mp, n_kf, stride, mp_live, n_mp, kf_id, kp_x, kp_y, kp_octave, kp_depth, kf_desc_base, cur, adj, matched, n_kp1, n_kp2, new_rows,
                                            n_new, n_levels, &lists, cap_rows, cap_obs, out_i, out_i, out_i, why, n);
    }
};

struct CreateBind {
    static constexpr const char *fn = "ms_create_points_bind_check";
    int n_kf = 5, stride = 8, n_mp = 10, n_pool = 40, cur = 1, adj = 3, n_matches = 4, n_kp1 = 6, n_kp2 = 8;
    const uint32_t *desc = mp_desc;
    const int32_t *n_created = out_i;
    ms_obs_lists lists = all_lists();
    int call(char *why, size_t n) {
        return ms_create_points_bind_check(kf_mp, n_kf, stride, mp_flags, mp_live, desc, n_obs_tab, mp_track, n_mp, desc_pool, n_pool, cur, adj, &lists, out_i, out_i, n_matches,
                                           n_kp1, n_kp2, out_b, out_b, out_i, out_i, out_i, n_created, why, n);
    }
};

struct Unbound {
    static constexpr const char *fn = "ms_unbound_mask_check";
    int n_kf = 5, stride = 8, n_mp = 10, n_slots = 3;
    int32_t slots3[3] = {1, 3, 0}, n_kp3[3] = {6, 8, 0};
    uint8_t *usable3[3] = {out_b, out_b, nullptr};
    const int32_t *slots = slots3, *n_kp = n_kp3;
    uint8_t *const *usable = usable3;
    int call(char *why, size_t n) { return ms_unbound_mask_check(kf_mp, n_kf, stride, n_mp, slots, n_kp, usable, n_slots, why, n); }
};

struct Bound {
    static constexpr const char *fn = "ms_bound_mask_check";
    int n_kf = 5, stride = 8, n_mp = 10, slot = 1, n_kp = 6;
    const uint8_t *skip = out_b;
    const int32_t *tab = kf_mp;
    int call(char *why, size_t n) { return ms_bound_mask_check(tab, n_kf, stride, n_mp, slot, n_kp, skip, why, n); }
};

struct SearchBind {
    static constexpr const char *fn = "ms_search_bind_check";
    int n_kf = 5, stride = 8, n_mp = 10, n_kp = 6, first = 2, count = 5, n_kept = 3, slot = 1;
    int32_t mp_index[8] = {0, 1, 2, 3, 4, 5, 6, 7};
    const int32_t *counts = out_i;
    int call(char *why, size_t n) {
        return ms_search_bind_check(kf_mp, n_kf, stride, mp_live, n_obs_tab, n_mp, out_i, out_f, out_f, out_f, nullptr, nullptr, q_desc, out_i, out_h, out_i, out_i, out_b, out_f,
                                    out_f, out_i, t_desc, out_i, n_kp, mp_index, first, count, n_kept, slot, out_i, counts, why, n);
    }
};

struct WindowLists {
    static constexpr const char *fn = "ms_ba_window_lists_check";
    int n_kf = 5, n_mp = 10, n_rows = 3, n_obs = 5, n_local = 3, current = 0, n_levels = 3, cap_point = 8, cap_edge = 16;
    int32_t local[3] = {1, 3, 0};
    float levels[3] = {1.f, 1.44f, 2.0736f};
    const double *pose = out_d;
    ms_obs_lists lists = all_lists();
    ms_ba_window_dev window = {out_i, out_i, out_i};
    int call(char *why, size_t n) {
        return ms_ba_window_lists_check(kf_pose, n_kf, mp_pos, n_mp, &lists, n_rows, n_obs, local, n_local, current, cams, kf_focal, levels, n_levels, pose, out_d, out_i, out_i,
                                        out_d, out_d, cap_point, cap_edge, &window, out_i, out_i, why, n);
    }
};

struct WindowApply {
    static constexpr const char *fn = "ms_ba_window_apply_check";
    int n_kf = 5, stride = 8, n_mp = 10, n_pose = 3, n_edge = 5, n_rows = 3, n_local = 3, current = 0, mode = MS_BA_APPLY_LOCAL, cap_erased = 8;
    int32_t local[3] = {1, 3, 0};
    const double *pose = out_d;
    ms_ba_window_dev window = {out_i, out_i, out_i};
    int call(char *why, size_t n) {
        return ms_ba_window_apply_check(kf_mp, n_kf, stride, mp_pos, mp_flags, n_obs_tab, n_mp, kf_pose, pose, n_pose, out_d, out_d, &window, n_edge, out_i, n_rows, local, n_local,
                                        current, mode, out_i, cap_erased, out_i, out_i, why, n);
    }
};

// the three loop-closure checks: the current keyframe in slot 1 with 6 keypoints; candidates in slots 3, 0 and 4 with 8, 0 and 5 keypoints
struct LoopMask {
    static constexpr const char *fn = "ms_loop_usable_mask_check";
    int n_kf = 5, stride = 8, n_mp = 10, n_slots = 3;
    const uint8_t *flags = mp_flags;
    int32_t slots[3] = {1, 3, 0}, n_kp[3] = {6, 8, 0}, require[3] = {0, 1, 1};
    const int32_t *p_slots = slots;
    uint8_t *usable[3] = {out_b, out_b, nullptr};
    int32_t *tri_row[3] = {out_i, nullptr, nullptr};
    int call(char *why, size_t n) { return ms_loop_usable_mask_check(kf_mp, n_kf, stride, flags, mp_live, n_mp, p_slots, n_kp, require, usable, tri_row, n_slots, why, n); }
};

struct LoopPairs {
    static constexpr const char *fn = "ms_loop_pairs_check";
    int n_kf = 5, stride = 8, n_mp = 10, cur = 1, n_kp_cur = 6, n_cand = 3, n_levels = 3, cap_pairs = 18;
    int32_t cand_slot[3] = {3, 0, 4}, n_kp_cand[3] = {8, 0, 5};
    const int32_t *matched[3] = {out_i, out_i, out_i};
    float levels[3] = {1.f, 1.44f, 2.0736f};
    const double *pose = kf_pose;
    int call(char *why, size_t n) {
        return ms_loop_pairs_check(kf_mp, n_kf, stride, mp_live, mp_pos, n_mp, pose, kp_octave, cur, n_kp_cur, cand_slot, n_kp_cand, matched, n_cand, levels, n_levels, cap_pairs,
                                   out_i, out_i, out_i, out_i, out_i, out_d, out_d, out_f, out_f, out_d, out_d, out_i, why, n);
    }
};

struct LoopSim3 {
    static constexpr const char *fn = "ms_loop_sim3_lists_check";
    int n_kf = 5, stride = 8, n_mp = 10, cur = 1, n_kp_cur = 6, n_cand = 3, n_levels = 3;
    int32_t cand_slot[3] = {3, 0, 4}, n_kp_cand[3] = {8, 0, 5}, match_start[4] = {0, 2, 2, 5};
    float levels[3] = {1.f, 1.44f, 2.0736f};
    const double *pose = kf_pose;
    int call(char *why, size_t n) {
        return ms_loop_sim3_lists_check(kf_mp, n_kf, stride, mp_live, mp_pos, n_mp, pose, kp_x, kp_y, kp_octave, cur, n_kp_cur, cand_slot, n_kp_cand, n_cand, cams, levels, n_levels,
                                        out_i, out_i, match_start, out_d, out_d, out_d, out_d, out_f, out_f, out_i, out_i, why, n);
    }
};

struct PoseTables {
    static constexpr const char *fn = "ms_pose_tables_solve_check";
    int n_kf = 5, stride = 8, n_mp = 10;
    ms_pose_tables_frame f;
    const ms_pose_tables_frame *p_f = &f;
    ms_pose_tables_out out;
    PoseTables() {
        std::memset(&f, 0, sizeof(f));
        std::memset(&out, 0, sizeof(out));
        f.slot = 1; f.prev_slot = 0; f.n_kp = 6; f.cam = cams[0]; f.focal = 500; f.edge_meas[3] = 1.0;
        for (int i = 0; i < 6; ++i) f.edge_info[7 * i] = 1.0;
        f.min_visible = 10; f.max_iters = 5; f.huber_delta = 2.0;
    }
    int call(char *why, size_t n) { return ms_pose_tables_solve_check(kf_mp, n_kf, stride, mp_flags, mp_live, mp_pos, n_mp, kp_x, kp_y, kp_octave, kf_pose, p_f, &out, why, n); }
};

}  // namespace

int main() {
    for (int i = 0; i < 40; ++i) kf_mp[i] = -1;
    for (int i = 0; i < kBig; ++i) { kf_id[i] = i; kf_t[i] = 0.1 * i; }
    for (ms_pinhole &c : cams) c = ms_pinhole{500.0, 510.0, 320.0, 240.0, 640, 480};

    CASE(Refresh, "accepted");
    CASE(Refresh, "every size zero", a.n_mp = a.n_kf = a.n_pool = a.n_rows = 0);
    CASE(Refresh, "negative size", a.n_pool = -1);
    CASE(Refresh, "no levels", a.n_levels = 0);
    CASE(Refresh, "missing array", a.p_rows = nullptr);
    CASE(Refresh, "unaligned descriptors", a.desc = mp_desc + 1);
    CASE(Refresh, "row outside", a.rows[1] = 10);
    CASE(Refresh, "last: row twice", a.rows[2] = 1);

    CASE(LoopCorrect, "accepted");
    CASE(LoopCorrect, "every size zero", a.n_kf = a.n_mp = a.n_corr = a.n_pts = 0);
    CASE(LoopCorrect, "negative size", a.n_corr = -1);
    CASE(LoopCorrect, "missing array", a.p_slot = nullptr);
    CASE(LoopCorrect, "lambda outside", a.lambda[2] = 1.5);
    CASE(LoopCorrect, "slot twice", a.slot[2] = 1);
    CASE(LoopCorrect, "last: row twice", a.row[2] = 2);

    CASE(Covis, "accepted");
    CASE(Covis, "every size zero", a.n_kf = a.n_mp = a.n_q = 0);
    CASE(Covis, "negative size", a.n_q = -1);
    CASE(Covis, "stride 0", a.stride = 0);
    CASE(Covis, "missing array", a.p_q = nullptr);
    TABLE_CAPS(Covis); STRIDE_CAP(Covis);
    CASE(Covis, "cap queries", a.n_q = MS_COVIS_MAX_QUERIES + 1; a.p_q = nullptr);
    CASE(Covis, "last: flags required", a.flags = nullptr);

    CASE(Union, "accepted");
    CASE(Union, "every size zero", a.n_kf = a.n_mp = a.n_list = a.n_u = 0);
    CASE(Union, "negative size", a.n_list = -1);
    CASE(Union, "stride 0", a.stride = 0);
    CASE(Union, "missing array", a.p_u = nullptr);
    TABLE_CAPS(Union); STRIDE_CAP(Union);
    CASE(Union, "flags required", a.flags = nullptr);
    CASE(Union, "last: list entry outside", a.list[1] = 5);

    CASE(Cull, "accepted");
    CASE(Cull, "every size zero", a.n_kf = a.n_mp = a.n_cand = 0);
    CASE(Cull, "negative size", a.n_cand = -1);
    CASE(Cull, "negative table size", a.n_kf = -1);
    CASE(Cull, "stride 0", a.stride = 0);
    CASE(Cull, "missing array", a.t = nullptr);
    TABLE_CAPS(Cull); STRIDE_CAP(Cull);
    CASE(Cull, "current slot outside", a.s.current_slot = 5);
    CASE(Cull, "last: candidate twice", a.cand[2] = 3);

    CASE(Tri, "accepted");
    CASE(Tri, "every size zero", a.n_mp = a.n_kf = a.n_rows = 0);
    CASE(Tri, "negative size", a.n_rows = -1);
    CASE(Tri, "mode", a.mode = 3);
    CASE(Tri, "missing array", a.p_rows = nullptr);
    CASE(Tri, "cap rows", a.n_rows = MS_TRI_MAX_ROWS + 1);
    CASE(Tri, "cap observations", a.n_rows = 1; a.obs_start[1] = MS_TRI_MAX_OBS + 1);
    CASE(Tri, "octave outside", a.obs_octave[4] = 3);
    CASE(Tri, "last: row twice", a.rows[2] = 4);

    CASE(ObsLists, "accepted");
    CASE(ObsLists, "accepted from a slot", a.sel.source = MS_OBS_FROM_SLOT; a.sel.slot = 3; a.sel.filter = MS_OBS_REFRESH);
    CASE(ObsLists, "every size zero", a.n_kf = a.n_mp = a.n_levels = a.cap_rows = a.cap_obs = 0; a.sel.n_in = 0);
    CASE(ObsLists, "negative size", a.cap_obs = -1);
    CASE(ObsLists, "negative table size", a.n_mp = -1);
    CASE(ObsLists, "stride 0", a.stride = 0);
    CASE(ObsLists, "missing array", a.p_sel = nullptr);
    TABLE_CAPS(ObsLists); STRIDE_CAP(ObsLists);
    CASE(ObsLists, "kf_id twice", a.n_kf = 5; kf_id[4] = 2);
    kf_id[4] = 4;
    CASE(ObsLists, "last: was_triangulated without flags", a.flags = nullptr);

    CASE(Tracked, "accepted");
    CASE(Tracked, "every size zero", a.n_kf = a.n_mp = a.n_pool = a.n_track = a.n_kp = a.n_new = 0);
    CASE(Tracked, "negative size", a.n_new = -1);
    CASE(Tracked, "stride 0", a.stride = 0);
    CASE(Tracked, "missing array", a.p_f = nullptr);
    CASE(Tracked, "track id outside", a.kp_track[2] = 106);
    CASE(Tracked, "track id twice", a.kp_track[5] = 100);
    CASE(Tracked, "last invalid: new row outside", a.new_rows[3] = 10);
    TABLE_CAPS(Tracked); STRIDE_CAP(Tracked);
    CASE(Tracked, "last: cap tracks", a.n_track = MS_TRACKED_MAX_WINDOW + 1);

    CASE(Finish, "accepted");
    CASE(Finish, "every size zero", a.n_rows = a.n_mp = a.n_checked = a.cap_refresh = 0);
    CASE(Finish, "negative size", a.n_checked = -1);
    CASE(Finish, "missing array", a.n_refresh = nullptr);
    CASE(Finish, "last invalid: unaligned descriptors", a.desc = mp_desc + 1);
    CASE(Finish, "cap rows", a.n_rows = MS_COVIS_MAX_STRIDE + 1; a.cap_refresh = 20000);
    CASE(Finish, "cap checked rows", a.n_checked = MS_COVIS_MAX_STRIDE + 1; a.cap_refresh = 20000);
    CASE(Finish, "cap map points", a.n_mp = MS_COVIS_MAX_MP);
    CASE(Finish, "last: cap refresh_rows", a.cap_refresh = 4);
    CASE(Finish, "not appended", a.cap_refresh = 4; a.append = 0);

    CASE(Fuse, "accepted");
    CASE(Fuse, "every size zero", a.n_kf = a.n_mp = a.n_track = a.n_entries = a.n_views = 0; a.source_slot = -1);
    CASE(Fuse, "negative size", a.n_views = -1);
    CASE(Fuse, "negative table size", a.n_track = -1);
    CASE(Fuse, "stride 0", a.stride = 0);
    CASE(Fuse, "missing array", a.counts = nullptr);
    TABLE_CAPS(Fuse); STRIDE_CAP(Fuse);
    CASE(Fuse, "cap tracks", a.n_track = MS_TRACKED_MAX_WINDOW + 1);
    CASE(Fuse, "cap views", a.n_views = MS_GATE_MAX_VIEWS + 1);
    CASE(Fuse, "cap entries", a.n_entries = MS_GATE_MAX_ENTRIES);
    CASE(Fuse, "slices overlap", a.views[1].first = 2);
    CASE(Fuse, "last: row twice in a view", a.mp_index[7] = 5);

    CASE(Pairs, "accepted");
    CASE(Pairs, "every size zero", a.n_kf = a.n_mp = a.n_track = a.n_pairs = 0);
    CASE(Pairs, "negative size", a.n_pairs = -1);
    CASE(Pairs, "stride 0", a.stride = 0);
    CASE(Pairs, "missing array", a.p_pairs = nullptr);
    TABLE_CAPS(Pairs); STRIDE_CAP(Pairs);
    CASE(Pairs, "cap tracks", a.n_track = MS_TRACKED_MAX_WINDOW + 1);
    CASE(Pairs, "cap pairs", a.n_pairs = MS_GATE_MAX_ENTRIES);
    CASE(Pairs, "last: row outside", a.pairs[3] = 10);

    CASE(CreateLists, "accepted");
    CASE(CreateLists, "every size zero", a.n_kf = a.n_mp = a.n_kp1 = a.n_kp2 = a.n_new = a.n_levels = a.cap_rows = a.cap_obs = 0);
    CASE(CreateLists, "negative size", a.n_kp2 = -1);
    CASE(CreateLists, "stride 0", a.stride = 0);
    CASE(CreateLists, "missing array", a.matched = nullptr);
    CASE(CreateLists, "same slot", a.adj = 1);
    CASE(CreateLists, "last invalid: new row outside", a.new_rows[2] = 10);
    CASE(CreateLists, "new row twice", a.new_rows[2] = 2);
    TABLE_CAPS(CreateLists);
    CASE(CreateLists, "last: cap stride", a.stride = MS_COVIS_MAX_STRIDE + 1);

    CASE(CreateBind, "accepted");
    CASE(CreateBind, "every size zero", a.n_kf = a.n_mp = a.n_pool = a.n_matches = a.n_kp1 = a.n_kp2 = 0);
    CASE(CreateBind, "negative size", a.n_matches = -1);
    CASE(CreateBind, "stride 0", a.stride = 0);
    CASE(CreateBind, "missing array", a.n_created = nullptr);
    CASE(CreateBind, "last invalid: unaligned descriptors", a.desc = mp_desc + 1);
    TABLE_CAPS(CreateBind); STRIDE_CAP(CreateBind);
    CASE(CreateBind, "last: cap matches", a.n_matches = MS_COVIS_MAX_STRIDE + 1);

    CASE(Unbound, "accepted");
    CASE(Unbound, "every size zero", a.n_kf = a.n_mp = a.n_slots = 0);
    CASE(Unbound, "negative size", a.n_slots = -1);
    CASE(Unbound, "stride 0", a.stride = 0);
    CASE(Unbound, "missing array", a.n_kp = nullptr);
    CASE(Unbound, "last invalid: missing mask of a slot", a.usable3[1] = nullptr);
    TABLE_CAPS(Unbound); STRIDE_CAP(Unbound);
    CASE(Unbound, "last: cap listed slots", a.n_slots = MS_COVIS_MAX_QUERIES + 1; a.slots = zeros_i; a.n_kp = zeros_i; a.usable = no_masks);

    CASE(Bound, "accepted");
    CASE(Bound, "every size zero", a.n_kf = a.n_mp = a.n_kp = 0);
    CASE(Bound, "negative size", a.n_kp = -1);
    CASE(Bound, "stride 0", a.stride = 0);
    CASE(Bound, "missing array", a.tab = nullptr);
    TABLE_CAPS(Bound); STRIDE_CAP(Bound);
    CASE(Bound, "keypoints beyond the stride", a.n_kp = 9);
    CASE(Bound, "last: missing skip", a.skip = nullptr);

    CASE(SearchBind, "accepted");
    CASE(SearchBind, "every size zero", a.n_kf = a.n_mp = a.n_kp = a.first = a.count = a.n_kept = 0);
    CASE(SearchBind, "nothing kept", a.n_mp = a.n_kp = a.first = a.count = a.n_kept = 0);
    CASE(SearchBind, "negative size", a.n_kept = -1);
    CASE(SearchBind, "stride 0", a.stride = 0);
    CASE(SearchBind, "missing array", a.counts = nullptr);
    TABLE_CAPS(SearchBind); STRIDE_CAP(SearchBind);
    CASE(SearchBind, "cap count", a.count = MS_GATE_MAX_ENTRIES);
    CASE(SearchBind, "cap first", a.first = MS_GATE_MAX_ENTRIES - 5);
    CASE(SearchBind, "last: entry outside", a.mp_index[6] = 10);

    CASE(WindowLists, "accepted");
    CASE(WindowLists, "every size zero", a.n_kf = a.n_mp = a.n_rows = a.n_obs = a.n_local = a.cap_point = a.cap_edge = 0);
    CASE(WindowLists, "negative size", a.cap_edge = -1);
    CASE(WindowLists, "missing array", a.pose = nullptr);
    CASE(WindowLists, "local slot twice", a.local[2] = 1);
    CASE(WindowLists, "last invalid: level_sigma_sq", a.levels[2] = 0.f);
    CASE(WindowLists, "cap slots", a.n_kf = MS_COVIS_MAX_KF + 1);
    CASE(WindowLists, "cap map points", a.n_mp = MS_COVIS_MAX_MP);
    CASE(WindowLists, "cap rows", a.n_rows = MS_TRI_MAX_ROWS + 1);
    CASE(WindowLists, "last: cap observations", a.n_obs = MS_TRI_MAX_OBS + 1);

    CASE(WindowApply, "accepted");
    CASE(WindowApply, "accepted for the neighbourhood", a.mode = MS_BA_APPLY_NEIGHBOR);
    CASE(WindowApply, "every size zero", a.n_kf = a.n_mp = a.n_pose = a.n_edge = a.n_rows = a.n_local = a.cap_erased = 0);
    CASE(WindowApply, "negative size", a.n_edge = -1);
    CASE(WindowApply, "stride 0", a.stride = 0);
    CASE(WindowApply, "missing array", a.pose = nullptr);
    CASE(WindowApply, "last invalid: current index", a.current = 3);
    TABLE_CAPS(WindowApply); STRIDE_CAP(WindowApply);
    CASE(WindowApply, "cap rows", a.n_rows = MS_TRI_MAX_ROWS + 1);
    CASE(WindowApply, "last: cap edges", a.n_edge = MS_TRI_MAX_OBS + 1);

    CASE(LoopMask, "accepted");
    CASE(LoopMask, "every size zero", a.n_kf = a.n_mp = a.n_slots = 0);
    CASE(LoopMask, "negative size", a.n_slots = -1);
    CASE(LoopMask, "stride 0", a.stride = 0);
    CASE(LoopMask, "missing array", a.p_slots = nullptr);
    TABLE_CAPS(LoopMask); STRIDE_CAP(LoopMask);
    CASE(LoopMask, "cap listed slots", a.n_slots = MS_COVIS_MAX_QUERIES + 1);
    CASE(LoopMask, "last: flags required", a.flags = nullptr);

    CASE(LoopPairs, "accepted");
    CASE(LoopPairs, "every size zero", a.n_kf = a.n_mp = a.n_kp_cur = a.n_cand = a.cap_pairs = 0);
    CASE(LoopPairs, "no candidates", a.n_cand = 0);
    CASE(LoopPairs, "negative size", a.cap_pairs = -1);
    CASE(LoopPairs, "negative table size", a.n_cand = -1);
    CASE(LoopPairs, "stride 0", a.stride = 0);
    CASE(LoopPairs, "missing array", a.pose = nullptr);
    TABLE_CAPS(LoopPairs); STRIDE_CAP(LoopPairs);
    CASE(LoopPairs, "cap candidates", a.n_cand = MS_LOOP_MAX_CANDIDATES + 1);
    CASE(LoopPairs, "candidate twice", a.cand_slot[2] = 3);
    CASE(LoopPairs, "missing match list", a.matched[1] = nullptr);
    CASE(LoopPairs, "last: level_sigma_sq", a.levels[2] = -1.f);

    CASE(LoopSim3, "accepted");
    CASE(LoopSim3, "every size zero", a.n_kf = a.n_mp = a.n_kp_cur = a.n_cand = 0);
    CASE(LoopSim3, "no candidates", a.n_cand = 0);
    CASE(LoopSim3, "negative size", a.n_cand = -1);
    CASE(LoopSim3, "stride 0", a.stride = 0);
    CASE(LoopSim3, "missing array", a.pose = nullptr);
    TABLE_CAPS(LoopSim3); STRIDE_CAP(LoopSim3);
    CASE(LoopSim3, "cap candidates", a.n_cand = MS_LOOP_MAX_CANDIDATES + 1);
    CASE(LoopSim3, "cap matches of a candidate", a.match_start[1] = a.match_start[2] = a.match_start[3] = 9);
    CASE(LoopSim3, "match_start descends", a.match_start[2] = 1);
    CASE(LoopSim3, "camera", cams[3].fy = -2.0);
    cams[3].fy = 510.0;
    CASE(LoopSim3, "last: level_sigma_sq", a.levels[1] = 0.f);

    CASE(PoseTables, "accepted");
    CASE(PoseTables, "accepted without a previous keyframe", a.f.prev_slot = -1);
    CASE(PoseTables, "every size zero", a.n_kf = a.n_mp = 0; a.f.n_kp = 0);
    CASE(PoseTables, "negative size", a.n_mp = -1);
    CASE(PoseTables, "negative keypoints", a.f.n_kp = -1);
    CASE(PoseTables, "stride 0", a.stride = 0);
    CASE(PoseTables, "missing array", a.p_f = nullptr);
    CASE(PoseTables, "last invalid: max_iters", a.f.max_iters = -1);
    TABLE_CAPS(PoseTables);
    CASE(PoseTables, "last: cap stride", a.stride = MS_COVIS_MAX_STRIDE + 1);
    return 0;
}
