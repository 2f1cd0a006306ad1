// bow.hip -- N3: vocabulary-tree descent of ORB descriptors on the device.
//
// BowIndex::transform (bow_index.cpp:59-93) copies every keypoint descriptor into a cv::Mat and calls
// DBoW2::TemplatedVocabulary<FORB>::transform(features, bowVector, featureVector, levelsup = 4) (:86-92), which walks each
// descriptor down the k-ary tree by smallest Hamming distance.  Here the walk is one kernel over all descriptors of a batch:
// 16 lanes per descriptor, one child per lane (32 B = two dwordx4 loads, the 16 lanes of a group read one contiguous run of
// 512 B because the tree is re-laid out with every node's children adjacent), xor + v_bcnt, and a 4-step DPP rotate-min over
// the group on the key (distance << 16 | child position): the FIRST child wins ties exactly like the strict `d < best_d` scan.
// The word/weight/node triple per descriptor is all the device produces; the two std::maps (BowVector with its L1
// normalisation, FeatureVector) are assembled from it by the host mirror in feature order, which keeps the floating-point sums
// identical to the reference's.
#include "bow_descend.h"      // BowTree and ms_bow_vocab are in ms_internal.h, the walk in bow_descend.h: keyframe_admit.hip runs the same descent

namespace {

__global__ __launch_bounds__(256) void k_bow_descend(BowTree T, const uint4 *__restrict__ desc, int n, int levels_up,
                                                     int32_t *__restrict__ out_word, double *__restrict__ out_weight, int32_t *__restrict__ out_node) {
    const int i = blockIdx.x * 16 + (threadIdx.x >> 4);
    bow_descend(T, desc, i, i < n, levels_up, out_word, out_weight, out_node);
}

}  // namespace

extern "C" {

int ms_bow_vocab_create(ms_ctx *c, int n_nodes, const int32_t *parent, const uint32_t *node_desc, const double *node_weight,
                        const int32_t *node_word, int depth_levels, ms_bow_vocab **out) {
    if (!c || !out || n_nodes < 1 || !parent || !node_desc || !node_weight || !node_word || depth_levels < 0) return MS_ERR_INVALID;
    // children in ascending node id (the order DBoW2 attaches them while loading / building); parents must precede children
    std::vector<int32_t> n_child((size_t)n_nodes, 0), first((size_t)n_nodes, 0), fill((size_t)n_nodes, 0), child((size_t)n_nodes, 0);
    for (int i = 1; i < n_nodes; ++i) {
        if (parent[i] < 0 || parent[i] >= i) return ms_fail(c, MS_ERR_INVALID, "bow vocabulary: parent of node %d is %d (must be an earlier node)", i, parent[i]);
        n_child[(size_t)parent[i]]++;
    }
    int max_children = 0;
    for (int i = 0; i < n_nodes; ++i) max_children = n_child[(size_t)i] > max_children ? n_child[(size_t)i] : max_children;
    if (max_children > 65535) return ms_fail(c, MS_ERR_CAPACITY, "bow vocabulary: a node has %d children (max 65535)", max_children);
    for (int i = 1; i < n_nodes; ++i) first[(size_t)i] = first[(size_t)i - 1] + n_child[(size_t)i - 1];
    for (int i = 1; i < n_nodes; ++i) child[(size_t)(first[(size_t)parent[i]] + fill[(size_t)parent[i]]++)] = i;
    // breadth-first renumbering: internal index -> original id, children of a node adjacent
    std::vector<int32_t> orig((size_t)n_nodes), inner_first((size_t)n_nodes, 0), inner_nc((size_t)n_nodes, 0), depth((size_t)n_nodes, 0);
    orig[0] = 0;
    int tail = 1, max_depth = 0;
    for (int head = 0; head < tail; ++head) {
        const int o = orig[(size_t)head];
        inner_first[(size_t)head] = tail; inner_nc[(size_t)head] = n_child[(size_t)o];
        for (int k = 0; k < n_child[(size_t)o]; ++k) { orig[(size_t)tail] = child[(size_t)(first[(size_t)o] + k)]; depth[(size_t)tail] = depth[(size_t)head] + 1; ++tail; }
        max_depth = depth[(size_t)head] > max_depth ? depth[(size_t)head] : max_depth;
    }
    if (tail != n_nodes) return ms_fail(c, MS_ERR_INVALID, "bow vocabulary: %d of %d nodes are reachable from the root", tail, n_nodes);
    const size_t N = (size_t)n_nodes;
    const size_t o_first = 0, o_nc = ms_align_up(o_first + 4 * N, 256), o_desc = ms_align_up(o_nc + 4 * N, 256), o_orig = ms_align_up(o_desc + 32 * N, 256),
                 o_word = ms_align_up(o_orig + 4 * N, 256), o_weight = ms_align_up(o_word + 4 * N, 256), total = o_weight + 8 * N;
    std::vector<uint8_t> host(total, 0);
    for (size_t k = 0; k < N; ++k) {
        const size_t o = (size_t)orig[k];
        reinterpret_cast<int32_t *>(host.data() + o_first)[k] = inner_first[k];
        reinterpret_cast<int32_t *>(host.data() + o_nc)[k] = inner_nc[k];
        for (int w = 0; w < 8; ++w) reinterpret_cast<uint32_t *>(host.data() + o_desc)[8 * k + (size_t)w] = node_desc[8 * o + (size_t)w];
        reinterpret_cast<int32_t *>(host.data() + o_orig)[k] = (int32_t)o;
        reinterpret_cast<int32_t *>(host.data() + o_word)[k] = node_word[o];
        reinterpret_cast<double *>(host.data() + o_weight)[k] = node_weight[o];
    }
    MS_HIP(c, hipSetDevice(c->device));
    ms_bow_vocab *v = new ms_bow_vocab();
    v->ctx = c; v->n_nodes = n_nodes; v->max_children = max_children;
    hipError_t e = hipMalloc(&v->slab, total);
    if (e == hipSuccess) e = hipMemcpy(v->slab, host.data(), total, hipMemcpyHostToDevice);
    if (e != hipSuccess) { if (v->slab) (void)hipFree(v->slab); delete v; return ms_fail(c, MS_ERR_HIP, "bow vocabulary upload failed: %s", hipGetErrorString(e)); }
    char *b = static_cast<char *>(v->slab);
    v->tree.first_child = reinterpret_cast<const int32_t *>(b + o_first);
    v->tree.n_children = reinterpret_cast<const int32_t *>(b + o_nc);
    v->tree.desc = reinterpret_cast<const uint4 *>(b + o_desc);
    v->tree.orig_id = reinterpret_cast<const int32_t *>(b + o_orig);
    v->tree.word = reinterpret_cast<const int32_t *>(b + o_word);
    v->tree.weight = reinterpret_cast<const double *>(b + o_weight);
    v->tree.depth_levels = depth_levels; v->tree.max_depth = max_depth + 1;
    *out = v;
    return MS_OK;
}

void ms_bow_vocab_destroy(ms_bow_vocab *v) {
    if (!v) return;
    if (v->slab) (void)hipFree(v->slab);
    delete v;
}

int ms_bow_transform(ms_ctx *c, const ms_bow_vocab *v, const uint32_t *desc, int n, int levels_up, int32_t *word, double *weight, int32_t *node) {
    MsRange range("Bow index transform");     // the reference's timer name, mapper_helpers.cpp:1193
    if (!c || !v || n < 0 || (n > 0 && (!desc || !word))) return MS_ERR_INVALID;
    if (n == 0) return MS_OK;
    if (reinterpret_cast<uintptr_t>(desc) % 16) return ms_fail(c, MS_ERR_INVALID, "bow transform: descriptors must be 16-byte aligned");
    MS_HIP(c, hipSetDevice(c->device));
    hipLaunchKernelGGL(k_bow_descend, dim3(ms_div_up(n, 16)), dim3(256), 0, c->stream, v->tree, reinterpret_cast<const uint4 *>(desc), n, levels_up, word, weight, node);
    MS_KERNEL_CHECK(c, "k_bow_descend");
    return MS_OK;
}

}  // extern "C"
