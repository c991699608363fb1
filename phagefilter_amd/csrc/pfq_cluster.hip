// pfq_cluster.hip — pfq_tree_recluster: average-linkage clustering of the leaf filters' chance-corrected similarities
// (include/pfq.h "re-clustering", DESIGN.md "Re-clustering").  Everything is an integer.
//
//   k_cluster_q      shared bits of a panel of leaf pairs -> q = floor(max(0, I m - A B) 2^20 / (U m - A B)), written to both
//                    halves of the score matrix
//   k_cluster_nn     per live row of the score matrix its best column under (S / w descending, node index ascending)
//   k_cluster_mutual / k_cluster_list   the pairs that chose each other, in ascending node index (the scan between them is
//                    launch_scan_u32)
//   k_cluster_add_rows / k_cluster_add_cols / k_cluster_retire   S(Z, W) = S(X, W) + S(Y, W) for the round's merges
//
// The score matrix S is u64 [n_slots][pitch]: a SLOT per cluster, not a row per node.  The leaves start in slots 0 .. L - 1;
// a merge leaves the new cluster in the slot of its left child and retires the slot of its right child, so the matrix never
// grows and a row stays one contiguous run that k_cluster_nn reads with 16-byte loads, retired columns included (they are
// skipped by their slot's meta word, not gathered around).  meta[slot] = (node index | CLUSTER_NONE, leaves of the cluster);
// slot_of[node] is the way back.  pitch is a multiple of 16 columns: rows start on 128-byte lines; the columns from L on are
// never live.
#include "pfq_kernels.h"

namespace pfq {

// (S1, w1, n1) before (S2, w2, n2): S1 / w1 > S2 / w2 as 128-bit products, on equality the smaller node index; an entry
// without a node loses to every other.
__device__ __forceinline__ bool cluster_before(unsigned long long s1, unsigned long long w1, uint32_t n1, unsigned long long s2, unsigned long long w2,
                                               uint32_t n2) {
    if (n1 == CLUSTER_NONE) return false;
    if (n2 == CLUSTER_NONE) return true;
    const unsigned long long h1 = __umul64hi(s1, w2), l1 = s1 * w2, h2 = __umul64hi(s2, w1), l2 = s2 * w1;
    if (h1 != h2) return h1 > h2;
    if (l1 != l2) return l1 > l2;
    return n1 < n2;
}

// One thread per pair of the panel: rows r0 .. r0 + n_r of the leaves against columns r0 .. r0 + n_c (the part of the
// panel on or above the diagonal is used, the matrix is mirrored).
__global__ void __launch_bounds__(256) k_cluster_q(const uint32_t *__restrict__ shared, const unsigned long long *__restrict__ pop, uint32_t r0, uint32_t n_r,
                                                   uint32_t n_c, unsigned long long m, unsigned long long *__restrict__ S, uint64_t pitch) {
    const uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (uint64_t)n_r * n_c) return;
    const uint32_t i = (uint32_t)(idx / n_c), j = (uint32_t)(idx % n_c);
    if (j <= i) return;
    const uint32_t gi = r0 + i, gj = r0 + j;
    const unsigned long long I = shared[idx], A = pop[gi], B = pop[gj], U = A + B - I;
    // A, B, I, U <= m < 2^32: every product is below 2^64
    const unsigned long long ab = A * B, im = I * m, den = U * m - ab;
    unsigned long long num = im > ab ? im - ab : 0ull, q = 0;
    if (den) {
        if (num >= den) q = 1ull << 20;  // (I = U: the filters are equal)
        else
            for (int s = 0; s < 20; ++s) {  // shift-and-subtract; the bit shifted out of the remainder is kept
                const unsigned long long carry = num >> 63;
                num <<= 1;
                q <<= 1;
                if (carry || num >= den) {
                    num -= den;
                    q |= 1ull;
                }
            }
    }
    S[(uint64_t)gi * pitch + gj] = q;
    S[(uint64_t)gj * pitch + gi] = q;
}

// One block per slot.  best[slot] = the slot of the row's best column, CLUSTER_NONE for a retired row and for the last cluster.
__global__ void __launch_bounds__(256) k_cluster_nn(const unsigned long long *__restrict__ S, uint64_t pitch, const uint2 *__restrict__ meta,
                                                    uint32_t *__restrict__ best) {
    __shared__ unsigned long long s_s[4];
    __shared__ uint32_t s_size[4], s_node[4], s_slot[4];
    const uint32_t r = blockIdx.x;
    const uint2 mr = meta[r];
    if (mr.x == CLUSTER_NONE) {  // (block-uniform)
        if (threadIdx.x == 0) best[r] = CLUSTER_NONE;
        return;
    }
    const ulonglong2 *row = reinterpret_cast<const ulonglong2 *>(S + (uint64_t)r * pitch);
    const uint4 *meta2 = reinterpret_cast<const uint4 *>(meta);
    unsigned long long bs = 0;
    uint32_t bsize = 1, bnode = CLUSTER_NONE, bslot = CLUSTER_NONE;
    for (uint32_t c2 = threadIdx.x; c2 < (uint32_t)(pitch >> 1); c2 += blockDim.x) {
        const ulonglong2 v = row[c2];
        const uint4 mc = meta2[c2];
        const uint32_t c = 2u * c2;
        if (c != r && cluster_before(v.x, (unsigned long long)mr.y * mc.y, mc.x, bs, (unsigned long long)mr.y * bsize, bnode))
            bs = v.x, bsize = mc.y, bnode = mc.x, bslot = c;
        if (c + 1u != r && cluster_before(v.y, (unsigned long long)mr.y * mc.w, mc.z, bs, (unsigned long long)mr.y * bsize, bnode))
            bs = v.y, bsize = mc.w, bnode = mc.z, bslot = c + 1u;
    }
    for (int d = 32; d > 0; d >>= 1) {
        const unsigned long long os = __shfl_down(bs, d);
        const uint32_t osize = __shfl_down(bsize, d), onode = __shfl_down(bnode, d), oslot = __shfl_down(bslot, d);
        if (cluster_before(os, (unsigned long long)mr.y * osize, onode, bs, (unsigned long long)mr.y * bsize, bnode))
            bs = os, bsize = osize, bnode = onode, bslot = oslot;
    }
    if (lane_id() == 0) {
        const uint32_t w = threadIdx.x >> 6;
        s_s[w] = bs, s_size[w] = bsize, s_node[w] = bnode, s_slot[w] = bslot;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (uint32_t w = 1; w < 4; ++w)
            if (cluster_before(s_s[w], (unsigned long long)mr.y * s_size[w], s_node[w], bs, (unsigned long long)mr.y * bsize, bnode))
                bs = s_s[w], bsize = s_size[w], bnode = s_node[w], bslot = s_slot[w];
        best[r] = bslot;
    }
}

// One thread per node made so far: flag[n] = node n is live, its best chose it back, and n is the smaller index of the two.
__global__ void __launch_bounds__(256) k_cluster_mutual(const uint32_t *__restrict__ slot_of, uint32_t n_nodes, const uint32_t *__restrict__ best,
                                                        const uint2 *__restrict__ meta, uint32_t *__restrict__ flag) {
    const uint32_t n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= n_nodes) return;
    const uint32_t s = slot_of[n];
    uint32_t f = 0;
    if (s != CLUSTER_NONE) {
        const uint32_t t = best[s];
        if (t != CLUSTER_NONE && best[t] == s && meta[t].x > n) f = 1;
    }
    flag[n] = f;
}

// pos = the exclusive scan of flag: the round's merges in ascending node index of their left child
__global__ void __launch_bounds__(256) k_cluster_list(const uint32_t *__restrict__ slot_of, uint32_t n_nodes, const uint32_t *__restrict__ best,
                                                      const uint2 *__restrict__ meta, const uint32_t *__restrict__ flag,
                                                      const unsigned long long *__restrict__ pos, const unsigned long long *__restrict__ S, uint64_t pitch,
                                                      ClusterMerge *__restrict__ list, uint32_t list_cap) {
    const uint32_t n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= n_nodes || !flag[n]) return;
    const unsigned long long k = pos[n];
    if (k >= list_cap) return;
    const uint32_t s = slot_of[n], t = best[s];
    list[k] = ClusterMerge{s, t, n, meta[t].x, S[(uint64_t)s * pitch + t]};
}

// blockIdx.y = the merge: row of the left child's slot += row of the right child's slot
__global__ void __launch_bounds__(256) k_cluster_add_rows(unsigned long long *__restrict__ S, uint64_t pitch, const ClusterMerge *__restrict__ list) {
    const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= pitch) return;
    const ClusterMerge mg = list[blockIdx.y];
    S[(uint64_t)mg.slot_a * pitch + c] += S[(uint64_t)mg.slot_b * pitch + c];
}

// blockIdx.x = a slot (after k_cluster_add_rows): in its row, column of every left child += column of the right child.  The
// merges of a round share no slot, so the threads of a block touch different words.
__global__ void __launch_bounds__(256) k_cluster_add_cols(unsigned long long *__restrict__ S, uint64_t pitch, const uint2 *__restrict__ meta,
                                                          const ClusterMerge *__restrict__ list, uint32_t n_merges) {
    const uint32_t r = blockIdx.x;
    if (meta[r].x == CLUSTER_NONE) return;
    unsigned long long *row = S + (uint64_t)r * pitch;
    for (uint32_t p = threadIdx.x; p < n_merges; p += blockDim.x) {
        const ClusterMerge mg = list[p];
        row[mg.slot_a] += row[mg.slot_b];
    }
}

// merge p of the round becomes node first_node + p, in the slot of its left child
__global__ void __launch_bounds__(256) k_cluster_retire(uint2 *__restrict__ meta, uint32_t *__restrict__ slot_of, const ClusterMerge *__restrict__ list,
                                                        uint32_t n_merges, uint32_t first_node) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_merges) return;
    const ClusterMerge mg = list[p];
    meta[mg.slot_a] = make_uint2(first_node + p, meta[mg.slot_a].y + meta[mg.slot_b].y);
    meta[mg.slot_b] = make_uint2(CLUSTER_NONE, 0u);
    slot_of[mg.node_a] = CLUSTER_NONE;
    slot_of[mg.node_b] = CLUSTER_NONE;
    slot_of[first_node + p] = mg.slot_a;
}

void launch_cluster_scores(const uint32_t *d_shared, const unsigned long long *d_pop, uint32_t r0, uint32_t n_r, uint32_t n_c, uint64_t nbits,
                           unsigned long long *d_S, uint64_t pitch, hipStream_t st) {
    const uint64_t n = (uint64_t)n_r * n_c;
    if (!n) return;
    hipLaunchKernelGGL(k_cluster_q, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, d_shared, d_pop, r0, n_r, n_c, (unsigned long long)nbits, d_S, pitch);
}

void launch_cluster_nearest(const unsigned long long *d_S, uint64_t pitch, const uint2 *d_meta, uint32_t n_slots, uint32_t *d_best, hipStream_t st) {
    if (!n_slots) return;
    hipLaunchKernelGGL(k_cluster_nn, dim3(n_slots), dim3(256), 0, st, d_S, pitch, d_meta, d_best);
}

void launch_cluster_mutual(const uint32_t *d_slot_of, uint32_t n_nodes, const uint32_t *d_best, const uint2 *d_meta, uint32_t *d_flag, hipStream_t st) {
    if (!n_nodes) return;
    hipLaunchKernelGGL(k_cluster_mutual, dim3((n_nodes + 255) / 256), dim3(256), 0, st, d_slot_of, n_nodes, d_best, d_meta, d_flag);
}

void launch_cluster_list(const uint32_t *d_slot_of, uint32_t n_nodes, const uint32_t *d_best, const uint2 *d_meta, const uint32_t *d_flag,
                         const unsigned long long *d_pos, const unsigned long long *d_S, uint64_t pitch, ClusterMerge *d_list, uint32_t list_cap,
                         hipStream_t st) {
    if (!n_nodes) return;
    hipLaunchKernelGGL(k_cluster_list, dim3((n_nodes + 255) / 256), dim3(256), 0, st, d_slot_of, n_nodes, d_best, d_meta, d_flag, d_pos, d_S, pitch, d_list,
                       list_cap);
}

void launch_cluster_merge(unsigned long long *d_S, uint64_t pitch, uint2 *d_meta, uint32_t *d_slot_of, uint32_t n_slots, const ClusterMerge *d_list,
                          uint32_t n_merges, uint32_t first_node, hipStream_t st) {
    if (!n_merges) return;
    hipLaunchKernelGGL(k_cluster_add_rows, dim3((uint32_t)((pitch + 255) / 256), n_merges), dim3(256), 0, st, d_S, pitch, d_list);
    hipLaunchKernelGGL(k_cluster_add_cols, dim3(n_slots), dim3(256), 0, st, d_S, pitch, d_meta, d_list, n_merges);
    hipLaunchKernelGGL(k_cluster_retire, dim3((n_merges + 255) / 256), dim3(256), 0, st, d_meta, d_slot_of, d_list, n_merges, first_node);
}

}  // namespace pfq
