// knn.h — K nearest neighbours (ured_knn_fwd / ured_knn_bwd), part of the nn.hip code object:
// included from nn.hip, shares its sqd() (the contract distance), its LDS tile size, its
// debug-bounds word (file id 2) and the ured_dbg_nn accessor.
//
// Row i of sample b lists the min(K, len2) valid p2 points with the smallest (distance, index),
// ascending in that lexicographic order (lowest index on ties, chamfer3D.cu:36-69,126), the
// remaining slots and every slot of a row i >= len1 hold (0, 0). Distances are compared through
// their bit patterns: a contract distance is never negative, so the unsigned order of the bits
// is the float order, +inf included, and the all-ones word sorts above every real distance.
//
// Streaming path (K <= 32): one thread per query, refs staged through LDS in SoA tiles as in
//   nn_fwd_kernel; the thread keeps its KT = next power of two >= K best as a sorted list in
//   registers (KT a template parameter, the insertion chain unrolled with compile-time indices).
//   The hot loop is one compare against the current worst; the chain runs only when it passes.
//   Refs come in ascending index order, the compare is strict and the insertion goes after equal
//   entries: the tie rule without an index compare.
// Selection path (32 < K <= 1024, m <= 4096): one workgroup per query writes the keys
//   (bits(dist) << 32) | index to LDS, padded to a power of two with all-ones keys, sorts them
//   (bitonic.h, the sort of occ.hip) and stores the first K.
// Backward: gather form, no float atomics. A query sums its own K terms in ascending k; a p2
//   point finds its terms by streaming the n*K (query, slot) entries through LDS in ascending
//   (i, k) order, each wave compacting the entries that target its own 64 points (the scheme of
//   nn_bwd_kernel with n*K pairs instead of n). Every element of both gradients is written.
#pragma once
#include "bitonic.h"

namespace {

constexpr int KNN_T = 64;            // threads (= queries) per block of the streaming path
constexpr int KNN_SEL_T = 256;       // threads per block of the selection path
constexpr int KNN_MAX_K = 1024;
constexpr int KNN_STREAM_K = 32;     // largest K of the streaming path
constexpr int KNN_SEL_M = 4096;      // largest m of the selection path (32 KiB of keys)

struct KnnArgs {
    const float* p1; const float* p2;    // [b,n,3], [b,m,3]
    const int* len1; const int* len2;    // [b] or nullptr
    int n, m, K;
    float* dists; int* idx;              // [b,n,K]
};

// valid length of sample b: lens[b] clamped into [0, cap] (cap when there is no table)
__device__ __forceinline__ int knn_len(const int* lens, int b, int cap) {
    return lens ? min(max(lens[b], 0), cap) : cap;
}

// (dn, in) into the ascending list d / id, after every entry <= dn; the last entry drops out.
// Called only with dn < d[KT - 1].
template <int KT>
__device__ __forceinline__ void knn_insert(unsigned (&d)[KT], int (&id)[KT], unsigned dn, int in) {
#pragma unroll
    for (int j = KT - 1; j > 0; --j) {
        const bool shift = d[j - 1] > dn;      // entry j-1 moves up to j
        const bool here = d[j] > dn;           // (else) the first entry above dn: the new one lands here
        id[j] = shift ? id[j - 1] : (here ? in : id[j]);
        d[j] = shift ? d[j - 1] : (here ? dn : d[j]);
    }
    const bool here = d[0] > dn;
    id[0] = here ? in : id[0];
    d[0] = here ? dn : d[0];
}

// RS groups of G = KNN_T / RS threads share the block's G queries: group g takes the g-th
// SUB = NN_TILE / RS refs of every tile (ascending indices within a group, so the tie rule holds
// there), and the RS partial lists are merged in LDS as 64-bit keys (bits(dist) << 32) | index.
// The keys of real entries are unique, so the merged list does not depend on the split.
template <int KT, int RS>
__global__ __launch_bounds__(KNN_T) void knn_stream_kernel(KnnArgs A) {
    constexpr int G = KNN_T / RS;            // queries per block
    constexpr int SUB = NN_TILE / RS;        // refs per group and tile (a multiple of 4)
    __shared__ __attribute__((aligned(16))) float sx[NN_TILE];
    __shared__ __attribute__((aligned(16))) float sy[NN_TILE];
    __shared__ __attribute__((aligned(16))) float sz[NN_TILE];
    __shared__ unsigned long long mkeys[RS > 1 ? KNN_T * KT : 1];
    const int b = blockIdx.y, t = threadIdx.x, g = t / G, u = t % G;
    const int len1 = knn_len(A.len1, b, A.n), len2 = knn_len(A.len2, b, A.m);
    const int q0 = blockIdx.x * G, qi = q0 + u;
    float* od = A.dists + ((size_t)b * A.n + qi) * A.K;
    int* oi = A.idx + ((size_t)b * A.n + qi) * A.K;
    if (q0 >= len1) {                        // uniform per block: padded rows only
        if (g == 0 && qi < A.n)
            for (int k = 0; k < A.K; ++k) { od[k] = 0.f; oi[k] = 0; }
        return;
    }
    const bool valid = qi < len1;
    const int qc = valid ? qi : len1 - 1;    // clamp: duplicate work, result discarded
    const float* qp = A.p1 + 3 * ((size_t)b * A.n + qc);
    const float qx = qp[0], qy = qp[1], qz = qp[2];
    unsigned d[KT];
    int id[KT];
#pragma unroll
    for (int k = 0; k < KT; ++k) { d[k] = ~0u; id[k] = 0; }

    const float* R = A.p2 + 3 * (size_t)b * A.m;
    for (int t0 = 0; t0 < len2; t0 += NN_TILE) {
        const int tn = min(NN_TILE, len2 - t0);
        URED_DBG_CHECK(t0 + tn <= A.m);
        __syncthreads();
        for (int i = t; i < tn; i += KNN_T) {
            const float* p = R + 3 * (size_t)(t0 + i);
            sx[i] = p[0]; sy[i] = p[1]; sz[i] = p[2];
        }
        __syncthreads();
        const int base = g * SUB;                        // this group's part of the tile
        const int sub_n = min(SUB, max(0, tn - base));
        URED_DBG_CHECK(base + sub_n <= NN_TILE);
        const int n4 = sub_n >> 2;
        for (int r4 = 0; r4 < n4; ++r4) {
            const float4 X = *reinterpret_cast<const float4*>(sx + base + 4 * r4);
            const float4 Y = *reinterpret_cast<const float4*>(sy + base + 4 * r4);
            const float4 Z = *reinterpret_cast<const float4*>(sz + base + 4 * r4);
            const unsigned u0 = __float_as_uint(sqd(qx, qy, qz, X.x, Y.x, Z.x));
            const unsigned u1 = __float_as_uint(sqd(qx, qy, qz, X.y, Y.y, Z.y));
            const unsigned u2 = __float_as_uint(sqd(qx, qy, qz, X.z, Y.z, Z.z));
            const unsigned u3 = __float_as_uint(sqd(qx, qy, qz, X.w, Y.w, Z.w));
            const int r = t0 + base + 4 * r4;
            if (u0 < d[KT - 1]) knn_insert<KT>(d, id, u0, r);
            if (u1 < d[KT - 1]) knn_insert<KT>(d, id, u1, r + 1);
            if (u2 < d[KT - 1]) knn_insert<KT>(d, id, u2, r + 2);
            if (u3 < d[KT - 1]) knn_insert<KT>(d, id, u3, r + 3);
        }
        for (int r = base + 4 * n4; r < base + sub_n; ++r) {
            const unsigned v = __float_as_uint(sqd(qx, qy, qz, sx[r], sy[r], sz[r]));
            if (v < d[KT - 1]) knn_insert<KT>(d, id, v, t0 + r);
        }
    }

    if constexpr (RS > 1) {
        // the groups' lists to LDS; group 0 merges the RS sorted lists of its query (an empty
        // slot's key, all-ones distance with index 0, sorts after every real key)
#pragma unroll
        for (int k = 0; k < KT; ++k) mkeys[(g * G + u) * KT + k] = ((unsigned long long)d[k] << 32) | (unsigned)id[k];
        __syncthreads();
        if (g != 0) return;
        int head[RS];
#pragma unroll
        for (int h = 0; h < RS; ++h) head[h] = 0;
#pragma unroll
        for (int k = 0; k < KT; ++k) {
            unsigned long long best = ~0ull;
            int bh = 0;
#pragma unroll
            for (int h = 0; h < RS; ++h) {
                const unsigned long long v = head[h] < KT ? mkeys[(h * G + u) * KT + head[h]] : ~0ull;
                if (v < best) { best = v; bh = h; }
            }
#pragma unroll
            for (int h = 0; h < RS; ++h) head[h] += (bh == h) ? 1 : 0;
            d[k] = (unsigned)(best >> 32);
            id[k] = (int)(unsigned)best;
        }
    }

    if (qi >= A.n) return;
    const int cnt = valid ? min(A.K, len2) : 0;
#pragma unroll
    for (int k = 0; k < KT; ++k) {
        if (k < A.K) {
            const bool ok = k < cnt;
            URED_DBG_CHECK(!ok || (unsigned)id[k] < (unsigned)len2);
            od[k] = ok ? __uint_as_float(d[k]) : 0.f;
            oi[k] = ok ? id[k] : 0;
        }
    }
}

__global__ __launch_bounds__(KNN_SEL_T) void knn_select_kernel(KnnArgs A) {
    __shared__ unsigned long long keys[KNN_SEL_M];
    const int b = blockIdx.y, i = blockIdx.x, t = threadIdx.x;
    const int len1 = knn_len(A.len1, b, A.n), len2 = knn_len(A.len2, b, A.m);
    float* od = A.dists + ((size_t)b * A.n + i) * A.K;
    int* oi = A.idx + ((size_t)b * A.n + i) * A.K;
    if (i >= len1 || len2 <= 0) {            // uniform per block
        for (int k = t; k < A.K; k += KNN_SEL_T) { od[k] = 0.f; oi[k] = 0; }
        return;
    }
    int P2 = 2;
    while (P2 < len2) P2 <<= 1;
    URED_DBG_CHECK(P2 <= KNN_SEL_M);
    if (P2 > KNN_SEL_M) return;              // the host check keeps m <= KNN_SEL_M
    const float* qp = A.p1 + 3 * ((size_t)b * A.n + i);
    const float qx = qp[0], qy = qp[1], qz = qp[2];
    const float* R = A.p2 + 3 * (size_t)b * A.m;
    for (int j = t; j < P2; j += KNN_SEL_T) {
        unsigned long long key = ~0ull;
        if (j < len2) {
            const float* p = R + 3 * (size_t)j;
            key = ((unsigned long long)__float_as_uint(sqd(qx, qy, qz, p[0], p[1], p[2])) << 32) | (unsigned)j;
        }
        keys[j] = key;
    }
    ured::bitonic_sort_u64<KNN_SEL_T>(keys, P2, t);
    const int cnt = min(A.K, len2);
    for (int k = t; k < A.K; k += KNN_SEL_T) {
        float dv = 0.f;
        int iv = 0;
        if (k < cnt) {
            const unsigned long long key = keys[k];
            dv = __uint_as_float((unsigned)(key >> 32));
            iv = (int)(unsigned)key;
            URED_DBG_CHECK((unsigned)iv < (unsigned)len2);
        }
        od[k] = dv;
        oi[k] = iv;
    }
}

struct KnnBwdArgs {
    const float* p1; const float* p2; const int* len1; const int* len2;
    int n, m, K;
    const float* gd; const int* idx;     // [b,n,K]
    float* g1; float* g2;                // [b,n,3], [b,m,3]
};

// grad_p1: one thread per query, its own terms in ascending k
__global__ __launch_bounds__(NN_THREADS) void knn_bwd_q_kernel(KnnBwdArgs A) {
    const int b = blockIdx.y, i = blockIdx.x * NN_THREADS + threadIdx.x;
    if (i >= A.n) return;
    const int len1 = knn_len(A.len1, b, A.n), len2 = knn_len(A.len2, b, A.m);
    const int cnt = i < len1 ? min(A.K, len2) : 0;
    const float* qp = A.p1 + 3 * ((size_t)b * A.n + i);
    const float px = qp[0], py = qp[1], pz = qp[2];
    const float* R = A.p2 + 3 * (size_t)b * A.m;
    const size_t e0 = ((size_t)b * A.n + i) * A.K;
    float ax = 0.f, ay = 0.f, az = 0.f;
    for (int k = 0; k < cnt; ++k) {
        int j = A.idx[e0 + k];
        URED_DBG_CHECK((unsigned)j < (unsigned)len2);
        j = min(max(j, 0), len2 - 1);        // a foreign index reads a valid point
        const float* r = R + 3 * (size_t)j;
        const float g = A.gd[e0 + k] * 2.f;
        ax += g * (px - r[0]); ay += g * (py - r[1]); az += g * (pz - r[2]);
    }
    float* o = A.g1 + 3 * ((size_t)b * A.n + i);
    o[0] = ax; o[1] = ay; o[2] = az;
}

// grad_p2: one thread per p2 point; the len1 * K entries e = i * K + k streamed in ascending order
__global__ __launch_bounds__(NN_THREADS) void knn_bwd_r_kernel(KnnBwdArgs A) {
    __shared__ int sidx[NN_TILE];
    __shared__ float sg[NN_TILE], sx[NN_TILE], sy[NN_TILE], sz[NN_TILE];
    __shared__ int slist[(NN_THREADS / 64) * NN_TILE];   // per-wave compacted entry lists
    const int b = blockIdx.y, j0 = blockIdx.x * NN_THREADS, j = j0 + threadIdx.x;
    const int len1 = knn_len(A.len1, b, A.n), len2 = knn_len(A.len2, b, A.m);
    const int cnt = min(A.K, len2);
    const bool valid = j < len2;
    float px = 0.f, py = 0.f, pz = 0.f;
    if (valid) {
        const float* pj = A.p2 + 3 * ((size_t)b * A.m + j);
        px = pj[0]; py = pj[1]; pz = pj[2];
    }
    float ax = 0.f, ay = 0.f, az = 0.f;
    const int total = j0 < len2 ? len1 * A.K : 0;        // uniform per block; n * K < 2^31 (host check)
    const size_t eb = (size_t)b * A.n * A.K;
    const float* Q = A.p1 + 3 * (size_t)b * A.n;
    for (int t0 = 0; t0 < total; t0 += NN_TILE) {
        const int tn = min(NN_TILE, total - t0);
        __syncthreads();
        for (int e = threadIdx.x; e < NN_TILE; e += NN_THREADS) {
            int id = -1; float gg = 0.f, x = 0.f, y = 0.f, z = 0.f;
            if (e < tn) {
                const int E = t0 + e, i = E / A.K, k = E - i * A.K;
                if (k < cnt) {
                    id = A.idx[eb + E]; gg = A.gd[eb + E];
                    URED_DBG_CHECK((unsigned)id < (unsigned)len2);
                    x = Q[3 * (size_t)i]; y = Q[3 * (size_t)i + 1]; z = Q[3 * (size_t)i + 2];
                }
            }
            sidx[e] = id; sg[e] = gg; sx[e] = x; sy[e] = y; sz[e] = z;
        }
        __syncthreads();
        // as in nn_bwd_kernel: each wave compacts, in ascending e, the entries that land in its
        // own 64 points, then walks that list; the owner lane accumulates
        const int wv = threadIdx.x >> 6, ln = threadIdx.x & 63;
        const int jw0 = j0 + wv * 64;
        int* lst = slist + wv * NN_TILE;
        int c = 0;
        for (int c0 = 0; c0 < tn; c0 += 64) {
            const int e = c0 + ln;
            const int id = e < tn ? sidx[e] : -1;
            const bool pred = (unsigned)(id - jw0) < 64u;
            const unsigned long long mask = __ballot(pred);
            if (pred) lst[c + __popcll(mask & ((1ull << ln) - 1ull))] = e;
            c += __popcll(mask);
        }
        for (int q = 0; q < c; ++q) {
            const int e = lst[q];
            const bool own = sidx[e] == j;
            const float g = sg[e] * 2.f;
            const float nx = ax - g * (sx[e] - px);
            const float ny = ay - g * (sy[e] - py);
            const float nz = az - g * (sz[e] - pz);
            ax = own ? nx : ax; ay = own ? ny : ay; az = own ? nz : az;
        }
    }
    if (j < A.m) {
        float* o = A.g2 + 3 * ((size_t)b * A.m + j);
        o[0] = valid ? ax : 0.f; o[1] = valid ? ay : 0.f; o[2] = valid ? az : 0.f;
    }
}

// Ref split by the number of queries: one query per lane needs 2048 waves' worth of queries to
// put two waves on each of the 1024 SIMDs; below that the ref range is split 2 or 4 ways.
template <int KT>
void knn_launch_stream(const KnnArgs& a, int b, hipStream_t st) {
    const long long waves1 = ((long long)b * a.n + KNN_T - 1) / KNN_T;
    if (waves1 >= 2048)
        hipLaunchKernelGGL((knn_stream_kernel<KT, 1>), dim3((a.n + KNN_T - 1) / KNN_T, b), dim3(KNN_T), 0, st, a);
    else if (waves1 >= 1024)
        hipLaunchKernelGGL((knn_stream_kernel<KT, 2>), dim3((a.n + KNN_T / 2 - 1) / (KNN_T / 2), b), dim3(KNN_T), 0, st, a);
    else
        hipLaunchKernelGGL((knn_stream_kernel<KT, 4>), dim3((a.n + KNN_T / 4 - 1) / (KNN_T / 4), b), dim3(KNN_T), 0, st, a);
}

// the argument checks of both entry points (sizes and limits only: no device work, no pointers)
int knn_check(const char* who, int b, int n, int m, int K) {
    URED_REQUIRE(b >= 0 && n >= 0 && m >= 0, "%s: negative size (b=%d n=%d m=%d)", who, b, n, m);
    URED_REQUIRE(K >= 1 && K <= KNN_MAX_K, "%s: K %d outside [1, %d]", who, K, KNN_MAX_K);
    URED_REQUIRE(K <= KNN_STREAM_K || m <= KNN_SEL_M, "%s: K %d > %d needs m <= %d (got m %d)", who, K,
                 KNN_STREAM_K, KNN_SEL_M, m);
    URED_REQUIRE(b <= 65535, "%s: b %d exceeds 65535", who, b);
    URED_REQUIRE((long long)n * K < (1ll << 31), "%s: n * K = %lld exceeds 2^31 - 1", who, (long long)n * K);
    return 0;
}

}  // namespace

extern "C" {

int ured_knn_fwd(const float* p1, const float* p2, int b, int n, int m, int K, const int* lengths1,
                 const int* lengths2, float* dists, int* idx, void* stream) {
    ured::clear_error();
    if (const int rc = knn_check("ured_knn_fwd", b, n, m, K)) return rc;
    if (b == 0 || n == 0) return 0;
    URED_REQUIRE(p1 && (p2 || m == 0) && dists && idx, "ured_knn_fwd: null pointer");
    const KnnArgs a{p1, p2, lengths1, lengths2, n, m, K, dists, idx};
    hipStream_t st = (hipStream_t)stream;
    if (K <= 2) knn_launch_stream<2>(a, b, st);
    else if (K <= 4) knn_launch_stream<4>(a, b, st);
    else if (K <= 8) knn_launch_stream<8>(a, b, st);
    else if (K <= 16) knn_launch_stream<16>(a, b, st);
    else if (K <= KNN_STREAM_K) knn_launch_stream<32>(a, b, st);
    else hipLaunchKernelGGL(knn_select_kernel, dim3(n, b), dim3(KNN_SEL_T), 0, st, a);
    return ured::launch_status("ured_knn_fwd");
}

int ured_knn_bwd(const float* p1, const float* p2, int b, int n, int m, int K, const int* lengths1,
                 const int* lengths2, const float* grad_dists, const int* idx, float* grad_p1, float* grad_p2,
                 void* stream) {
    ured::clear_error();
    if (const int rc = knn_check("ured_knn_bwd", b, n, m, K)) return rc;
    if (b == 0 || (n == 0 && m == 0)) return 0;
    URED_REQUIRE((p1 || n == 0) && (p2 || m == 0) && (n == 0 || m == 0 || (grad_dists && idx)) &&
                 (grad_p1 || n == 0) && (grad_p2 || m == 0), "ured_knn_bwd: null pointer");
    const KnnBwdArgs a{p1, p2, lengths1, lengths2, n, m, K, grad_dists, idx, grad_p1, grad_p2};
    hipStream_t st = (hipStream_t)stream;
    if (n > 0)
        hipLaunchKernelGGL(knn_bwd_q_kernel, dim3((n + NN_THREADS - 1) / NN_THREADS, b), dim3(NN_THREADS), 0, st, a);
    if (m > 0)
        hipLaunchKernelGGL(knn_bwd_r_kernel, dim3((m + NN_THREADS - 1) / NN_THREADS, b), dim3(NN_THREADS), 0, st, a);
    return ured::launch_status("ured_knn_bwd");
}

}  // extern "C"
