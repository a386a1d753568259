// interp.hip — PointNet++ feature propagation (the reference's network/pointnet/
// pointnet2_utils.py:293-309): inverse-distance interpolation of coarse features over the K <= 3
// nearest coarse points, written together with the skip features as the point-major matrix the conv
// chain reads, and its backward. Plain pointers, the caller's stream, no allocation, no host sync,
// no device state, no float atomics; every limit is checked on the host before any device work.
//
// Contract (fp32, no FMA contraction: the file is built with -ffp-contract=off and spells the order
// out; the divisions are IEEE divisions): r_k = 1.0f / (d_k + 1e-8f), R = (r_0 + r_1) + r_2,
// w_k = r_k / R, out_c = ((w_0 * f_0c) + (w_1 * f_1c)) + w_2 * f_2c with f_k = points2[b, idx[b,n,k]]
// (K = 2: R = r_0 + r_1 and two terms; K = 1: w_0 = r_0 / r_0 = 1, out = f_0 bit for bit).
//
// ured_interp_fwd.  One workgroup per IP_R fine points: a first pass (one thread per point) forms
// the weights, writes them to w_out and leaves them with the coarse row numbers in LDS; then the
// threads walk the IP_R x (D1 + D2) tile, four channels per thread where D1 and D2 allow: a copy
// of points1 in columns 0..D1-1, the weighted sum of the K gathered rows of points2 after them.
//
// ured_interp_bwd.  Two launches.
//  - grad_points2: the scheme of group_bwd_kernel (csrc/group.hip) with a weight on each row. One
//    wave per (32 coarse points, 64 channels) of a cloud: it scans the cloud's N*K indices in
//    order, 64 at a time, picks the entries that land in its own points (a ballot, walked from its
//    lowest bit), and for each of them, in order, the lanes add w * g (a product, then an add) to the
//    point's accumulators in LDS. Sums run over ascending (n,k) in fp32 from 0, every output
//    element is written once, and a second run is bitwise equal.
//  - grad_d2: one wave per IB_P fine points. The lanes share the channels of the K dot products
//    A_k = sum_c g_c * f_kc, a butterfly leaves the sums in every lane, and lane k < K writes
//    grad_d2_k = -((r_k * w_k) * sum_{j != k} w_j * (A_k - A_j)), j ascending. This form has no
//    f_k - out (which is rounding noise where d_k = 0 and r_k = 1e8); K = 1 gives 0.
#include <hip/hip_runtime.h>
#include <cstdint>
#define URED_DBG_FILE 13
#include "ured_common.h"
#include "../../include/ured_hip.h"

namespace {

typedef unsigned long long u64;
typedef unsigned int u32;

constexpr int IP_T = 256;
constexpr int IP_R = 64;                              // most points of one forward workgroup
constexpr float IP_EPS = 1e-8f;

template <int V> struct Vec;
template <> struct Vec<1> { typedef float T; };
template <> struct Vec<4> { typedef float4 T; };

__device__ __forceinline__ float ip_axpy(float w, float f) { return w * f; }
__device__ __forceinline__ float4 ip_axpy(float w, float4 f) { return make_float4(w * f.x, w * f.y, w * f.z, w * f.w); }
__device__ __forceinline__ float ip_add(float a, float b) { return a + b; }
__device__ __forceinline__ float4 ip_add(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// rows: the points of one workgroup (<= IP_R); V: channels per thread (4 needs D1 % 4 == D2 % 4 == 0
// and 16-byte aligned pointers: host check)
template <int V>
__global__ __launch_bounds__(IP_T) void interp_fwd_kernel(const float* __restrict__ points2, const int* __restrict__ idx,
                                                          const float* __restrict__ d2, const float* __restrict__ points1,
                                                          int N, int S, int K, int D1, int D2, u32 BN, int rows,
                                                          float* __restrict__ out, float* __restrict__ w_out) {
    typedef typename Vec<V>::T T;
    __shared__ float sw[IP_R * 3];
    __shared__ u32 srow[IP_R * 3];                    // b * S + idx: the row of points2
    const int t = threadIdx.x;
    const u32 r0 = blockIdx.x * (u32)rows;            // B * N * (D1 + D2) < 2^31 (host check)
    if (t < rows && r0 + t < BN) {
        const u32 r = r0 + t, b = r / (u32)N;
        float rk[3] = {0.f, 0.f, 0.f}, R = 0.f;
        int id[3] = {0, 0, 0};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (k < K) {
                id[k] = idx[(size_t)r * K + k];
                URED_DBG_CHECK(id[k] >= 0 && id[k] < S);
                id[k] = min(max(id[k], 0), S - 1);    // a bad index reads a wrong row, never outside the table
                rk[k] = 1.0f / (d2[(size_t)r * K + k] + IP_EPS);
                R = k == 0 ? rk[0] : R + rk[k];
            }
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (k < K) {
                const float w = rk[k] / R;
                sw[t * 3 + k] = w;
                srow[t * 3 + k] = b * (u32)S + (u32)id[k];
                w_out[(size_t)r * K + k] = w;
            }
        }
    }
    __syncthreads();
    const int C = D1 + D2, Cv = C / V, D1v = D1 / V;
    const int tile = rows * Cv;                       // <= IP_R * C < 2^31
    for (int e = t; e < tile; e += IP_T) {
        const int rl = e / Cv, cv = e - rl * Cv;
        const u32 r = r0 + rl;
        if (r >= BN) break;                           // rows ascend with e
        T v;
        if (cv < D1v) {
            v = reinterpret_cast<const T*>(points1 + (size_t)r * D1)[cv];
        } else {
            const int c = cv - D1v;
            v = ip_axpy(sw[rl * 3], reinterpret_cast<const T*>(points2 + (size_t)srow[rl * 3] * D2)[c]);
            if (K > 1) v = ip_add(v, ip_axpy(sw[rl * 3 + 1], reinterpret_cast<const T*>(points2 + (size_t)srow[rl * 3 + 1] * D2)[c]));
            if (K > 2) v = ip_add(v, ip_axpy(sw[rl * 3 + 2], reinterpret_cast<const T*>(points2 + (size_t)srow[rl * 3 + 2] * D2)[c]));
        }
        URED_DBG_CHECK((size_t)r * C + (size_t)(cv + 1) * V <= (size_t)BN * C);
        reinterpret_cast<T*>(out + (size_t)r * C)[cv] = v;
    }
}

constexpr int GB_P = 32, GB_C = 64;                   // coarse points x channels of one wave
constexpr int GB_U = 4;                               // loads kept in flight: index batches, and g rows

__global__ __launch_bounds__(64) void interp_bwd_p2_kernel(const float* __restrict__ g, const int* __restrict__ idx,
                                                           const float* __restrict__ w, int N, int S, int K, int D1, int D2,
                                                           int tiles_s, float* __restrict__ grad_points2) {
    __shared__ float acc[GB_P * GB_C];                // column ln belongs to lane ln alone: no barrier anywhere
    const int ln = threadIdx.x, b = blockIdx.y;
    const int ts = blockIdx.x % tiles_s, tc = blockIdx.x / tiles_s;
    const int j0 = ts * GB_P, c = tc * GB_C + ln;
    const int C = D1 + D2, E = N * K;                 // N * K < 2^31 (host check)
    const bool cin = c < D2;
    const int* I = idx + (size_t)b * E;
    const float* Wt = w + (size_t)b * E;
    const float* G = g + (size_t)b * N * C + D1 + (cin ? c : 0);
#pragma unroll
    for (int p = 0; p < GB_P; ++p) acc[p * GB_C + ln] = 0.f;
    for (int e0 = 0; e0 < E; e0 += 64 * GB_U) {
        int pl[GB_U];
        float wl[GB_U];
#pragma unroll
        for (int u = 0; u < GB_U; ++u) {              // GB_U batches of 64 entries, loaded together
            const int e = e0 + 64 * u + ln;
            const int id = e < E ? I[e] : -1;
            URED_DBG_CHECK(e >= E || (id >= 0 && id < S));
            wl[u] = e < E ? Wt[e] : 0.f;
            pl[u] = id - j0;                          // id = -1 and j0 >= 0: never in [0, GB_P)
        }
#pragma unroll
        for (int u = 0; u < GB_U; ++u) {              // ... and walked in order
            u64 mask = __ballot((u32)pl[u] < (u32)GB_P);
            const int eb = e0 + 64 * u;
            while (mask) {                            // the wave's entries of this batch, ascending, GB_U at a time
                int l[GB_U];
                float v[GB_U];
#pragma unroll
                for (int q = 0; q < GB_U; ++q) {
                    l[q] = mask ? (int)__builtin_ctzll(mask) : -1;
                    mask &= mask - 1;                 // 0 stays 0
                }
#pragma unroll
                for (int q = 0; q < GB_U; ++q) {
                    URED_DBG_CHECK(l[q] < 0 || eb + l[q] < E);
                    v[q] = (l[q] >= 0 && cin) ? G[(size_t)((eb + l[q]) / K) * C] : 0.f;
                }
#pragma unroll
                for (int q = 0; q < GB_U; ++q) {
                    if (l[q] < 0) break;              // wave-uniform
                    const int p = __builtin_amdgcn_readlane(pl[u], l[q]);
                    const float wk = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(wl[u]), l[q]));
                    URED_DBG_CHECK(p >= 0 && p < GB_P);
                    const float term = wk * v[q];
                    acc[p * GB_C + ln] += term;
                }
            }
        }
    }
    if (!cin) return;
    for (int p = 0; p < GB_P; ++p) {
        const int j = j0 + p;
        if (j >= S) break;
        grad_points2[((size_t)b * S + j) * D2 + c] = acc[p * GB_C + ln];
    }
}

constexpr int IB_P = 4;                               // fine points of one wave
constexpr int IB_W = IP_T / 64;                       // waves of one workgroup

__global__ __launch_bounds__(IP_T) void interp_bwd_d2_kernel(const float* __restrict__ g, const float* __restrict__ points2,
                                                             const int* __restrict__ idx, const float* __restrict__ w,
                                                             const float* __restrict__ d2, int N, int S, int K, int D1,
                                                             int D2, u32 BN, float* __restrict__ grad_d2) {
    const int ln = threadIdx.x & 63;
    const u32 first = (blockIdx.x * (u32)IB_W + (threadIdx.x >> 6)) * (u32)IB_P;
    const int C = D1 + D2;
    for (int i = 0; i < IB_P; ++i) {
        const u32 r = first + i;
        if (r >= BN) return;                          // wave-uniform
        const u32 b = r / (u32)N;
        float wk[3] = {0.f, 0.f, 0.f}, dk[3] = {0.f, 0.f, 0.f}, A[3] = {0.f, 0.f, 0.f};
        const float* F[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            int id = 0;
            if (k < K) {
                id = idx[(size_t)r * K + k];
                URED_DBG_CHECK(id >= 0 && id < S);
                id = min(max(id, 0), S - 1);
                wk[k] = w[(size_t)r * K + k];
                dk[k] = d2[(size_t)r * K + k];
            }
            F[k] = points2 + ((size_t)b * S + id) * D2;
        }
        const float* Gr = g + (size_t)r * C + D1;
        for (int c = ln; c < D2; c += 64) {
            const float gc = Gr[c];
#pragma unroll
            for (int k = 0; k < 3; ++k)
                if (k < K) {
                    const float pr = gc * F[k][c];
                    A[k] += pr;
                }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
            for (int k = 0; k < 3; ++k) A[k] += __shfl_xor(A[k], o);
        }
        if (ln < K) {
            float s = 0.f;
            bool any = false;
            const float Ak = ln == 0 ? A[0] : (ln == 1 ? A[1] : A[2]);
            const float wme = ln == 0 ? wk[0] : (ln == 1 ? wk[1] : wk[2]);
            const float dme = ln == 0 ? dk[0] : (ln == 1 ? dk[1] : dk[2]);
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                if (j < K && j != ln) {
                    const float term = wk[j] * (Ak - A[j]);
                    s = any ? s + term : term;
                    any = true;
                }
            }
            const float rme = 1.0f / (dme + IP_EPS);
            grad_d2[(size_t)r * K + ln] = any ? -((rme * wme) * s) : 0.f;
        }
    }
}

int interp_check(const char* who, int B, int N, int S, int K, int D1, int D2) {
    URED_REQUIRE(B >= 0, "%s: negative size (B %d)", who, B);
    URED_REQUIRE(K >= 1 && K <= 3, "%s: K %d outside [1, 3]", who, K);
    URED_REQUIRE(N >= 1 && S >= 1, "%s: N %d and S %d must be at least 1", who, N, S);
    URED_REQUIRE(D2 >= 1 && D1 >= 0, "%s: D2 %d must be at least 1 and D1 %d non-negative", who, D2, D1);
    URED_REQUIRE(B <= 65535, "%s: B %d exceeds 65535", who, B);
    URED_REQUIRE((long long)B * N * ((long long)D1 + D2) < (1ll << 31), "%s: B * N * (D1 + D2) = %lld exceeds 2^31 - 1", who,
                 (long long)B * N * ((long long)D1 + D2));
    URED_REQUIRE((long long)B * S * D2 < (1ll << 31), "%s: B * S * D2 = %lld exceeds 2^31 - 1", who, (long long)B * S * D2);
    URED_REQUIRE((long long)N * K < (1ll << 31), "%s: N * K = %lld exceeds 2^31 - 1", who, (long long)N * K);
    return 0;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace

extern "C" {

int ured_interp_fwd(const float* points2, const int* idx, const float* d2, const float* points1, int B, int N, int S,
                    int K, int D1, int D2, float* out, float* w_out, void* stream) {
    ured::clear_error();
    if (const int rc = interp_check("ured_interp_fwd", B, N, S, K, D1, D2)) return rc;
    URED_REQUIRE((points1 != nullptr) == (D1 > 0), "ured_interp_fwd: points1 and D1 > 0 go together (D1 %d)", D1);
    if (B == 0) return 0;
    URED_REQUIRE(points2 && idx && d2 && out && w_out, "ured_interp_fwd: null pointer");
    const int C = D1 + D2;
    const bool vec = D1 % 4 == 0 && D2 % 4 == 0 && aligned16(points2) && aligned16(out) && aligned16(points1);
    const int Cv = vec ? C / 4 : C;
    int rows = (8 * IP_T) / Cv;                       // about 8 loads per thread
    rows = rows < 4 ? 4 : (rows > IP_R ? IP_R : rows);
    const u32 BN = (u32)B * (u32)N;
    const dim3 grid((BN + rows - 1) / rows);
    hipStream_t st = (hipStream_t)stream;
    if (vec)
        hipLaunchKernelGGL(interp_fwd_kernel<4>, grid, dim3(IP_T), 0, st, points2, idx, d2, points1, N, S, K, D1, D2, BN, rows,
                           out, w_out);
    else
        hipLaunchKernelGGL(interp_fwd_kernel<1>, grid, dim3(IP_T), 0, st, points2, idx, d2, points1, N, S, K, D1, D2, BN, rows,
                           out, w_out);
    return ured::launch_status("ured_interp_fwd");
}

int ured_interp_bwd(const float* grad_out, const float* points2, const int* idx, const float* w, const float* d2, int B,
                    int N, int S, int K, int D1, int D2, float* grad_points2, float* grad_d2, void* stream) {
    ured::clear_error();
    if (const int rc = interp_check("ured_interp_bwd", B, N, S, K, D1, D2)) return rc;
    if (B == 0) return 0;
    URED_REQUIRE(grad_out && points2 && idx && w && d2 && grad_points2 && grad_d2, "ured_interp_bwd: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const int tiles_s = (S + GB_P - 1) / GB_P, tiles_c = (D2 + GB_C - 1) / GB_C;   // tiles_s * tiles_c <= B*S*D2 / 2048 + ...
    hipLaunchKernelGGL(interp_bwd_p2_kernel, dim3((unsigned)tiles_s * (unsigned)tiles_c, B), dim3(64), 0, st, grad_out, idx, w,
                       N, S, K, D1, D2, tiles_s, grad_points2);
    const u32 BN = (u32)B * (u32)N;
    const u32 per = IB_W * IB_P;
    hipLaunchKernelGGL(interp_bwd_d2_kernel, dim3((BN + per - 1) / per), dim3(IP_T), 0, st, grad_out, points2, idx, w, d2, N,
                       S, K, D1, D2, BN, grad_d2);
    return ured::launch_status("ured_interp_bwd");
}

}  // extern "C"

URED_DBG_ACCESSOR(ured_dbg_interp)
