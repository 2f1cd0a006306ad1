// bow_descend.h -- the vocabulary-tree walk of bow.hip as device code that more than one kernel calls (ms_internal.h holds the tree's layout):
// k_bow_descend (bow.hip, ms_bow_transform) on a caller's descriptor array with a host count, k_admit_descend (keyframe_admit.hip) on
// an extractor view whose count is read on the device.  16 lanes per descriptor, one child per lane; bow.hip's header describes the walk.
#pragma once
#include "ms_internal.h"

__device__ __forceinline__ uint32_t bow_group_min16(uint32_t v) {      // min over each row of 16 lanes, result in every lane
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x121 /*row_ror:1*/, 0xf, 0xf, false));
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x122 /*row_ror:2*/, 0xf, 0xf, false));
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x124 /*row_ror:4*/, 0xf, 0xf, false));
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x128 /*row_ror:8*/, 0xf, 0xf, false));
    return v;
}

// Descriptor i of `desc` (16-byte aligned, 8 words each), walked by the 16 lanes threadIdx.x & ~15 .. | 15 of a 256-lane workgroup: every lane
// of the workgroup calls it, `live` = the group has a descriptor (a group without one walks nothing and writes nothing).  Lane 0 of the group
// writes out_word[i], and out_weight[i] / out_node[i] when they are given.
__device__ __forceinline__ void bow_descend(const BowTree &T, const uint4 *__restrict__ desc, int i, bool live, int levels_up, int32_t *__restrict__ out_word,
                                            double *__restrict__ out_weight, int32_t *__restrict__ out_node) {
    const int sub = threadIdx.x & 15;
    uint4 q0 = make_uint4(0, 0, 0, 0), q1 = q0;
    if (live) { q0 = desc[2 * (size_t)i]; q1 = desc[2 * (size_t)i + 1]; }
    const int nid_level = T.depth_levels - levels_up;
    int cur = 0, level = 0, nid = nid_level <= 0 ? 0 : -1;
    int nc = live ? T.n_children[0] : 0;
    const bool empty = nc == 0;
    // every group walks until its node has no children; max_depth bounds the loop for any tree the host accepted
    for (int step = 0; step < T.max_depth && __ballot(nc > 0) != 0; ++step) {
        if (nc > 0) {
            const int first = T.first_child[cur];
            uint32_t best = 0xFFFFFFFFu;
            for (int c0 = 0; c0 < nc; c0 += 16) {
                const int c = c0 + sub;
                uint32_t key = 0xFFFFFFFFu;
                if (c < nc) {
                    const uint4 a = T.desc[2 * (size_t)(first + c)], b = T.desc[2 * (size_t)(first + c) + 1];
                    const uint32_t d = __popc(a.x ^ q0.x) + __popc(a.y ^ q0.y) + __popc(a.z ^ q0.z) + __popc(a.w ^ q0.w) +
                                       __popc(b.x ^ q1.x) + __popc(b.y ^ q1.y) + __popc(b.z ^ q1.z) + __popc(b.w ^ q1.w);
                    key = (d << 16) | (uint32_t)c;
                }
                best = min(best, key);
            }
            best = bow_group_min16(best);
            cur = first + (int)(best & 0xFFFFu);
            ++level;
            if (level == nid_level) nid = cur;
            nc = T.n_children[cur];
        }
    }
    if (live && sub == 0) {
        if (empty) { out_word[i] = -1; if (out_weight) out_weight[i] = 0.0; if (out_node) out_node[i] = 0; return; }
        out_word[i] = T.word[cur];
        if (out_weight) out_weight[i] = T.weight[cur];
        if (out_node) out_node[i] = nid < 0 ? T.orig_id[cur] : (nid == 0 ? 0 : T.orig_id[nid]);
    }
}
