// group.hip — PointNet++ set abstraction primitives (the reference's network/pointnet/
// pointnet2_utils.py:63-138): farthest-point sampling, ball query, grouping and its backward.
// Plain pointers, the caller's stream, no allocation, no host sync, no device state, no float
// atomics; every limit is checked on the host before any device work.
//
// Contract distance (all kernels): d = ((dx*dx) + (dy*dy)) + (dz*dz) in fp32, dx = p.x - c.x,
// no FMA contraction (the file is built with -ffp-contract=off and spells the order out).
//
// ured_fps.  One workgroup per cloud, 64..1024 threads by N, thread t owns points t, t + T, ...
// (16 at most) with their running minima in registers. Per step: every thread updates its
// minima against the current centroid and forms the 64-bit key (bits(dmin) << 32) | ~j of its best
// point (distances are >= 0, so unsigned order is float order; ~j lets the lowest index win a
// tie); a butterfly over the wave leaves the wave's maximum in every lane, the owning lane
// publishes (key, x, y, z) in the wave's LDS slot, and after ONE barrier every thread takes the
// maximum over the slots and with it the next centroid's coordinates. The slots are double
// buffered: a slot set is rewritten two steps later, after the barrier of the step in between.
// Points j >= N of a thread hold dmin = 0 at (0,0,0) and an index above every real one: they are
// never updated (d < 0 is false) and lose every comparison, ties included.
//
// ured_ball_query.  One wave per query: the refs in index order, 64 at a time; a ballot of
// !(d > r2) and a prefix popcount append the hits in order; the scan stops once the row is full.
//
// ured_group_fwd.  One thread per output element of the point-major [B*S*K, C] matrix.
//
// ured_group_bwd.  One wave per (32 points, 64 channels) of a cloud: it scans the cloud's S*K
// indices in order, 64 at a time, picks the entries that land in its own points (a ballot, walked
// from its lowest bit), and for each of them, in order, the lanes add the entry's 64 channels of g
// (one coalesced row read) to the point's accumulators in LDS. Sums therefore run over ascending
// (s, k) in fp32 from 0, every output element is written once, and a second run is bitwise equal.
#include <hip/hip_runtime.h>
#define URED_DBG_FILE 12
#include "ured_common.h"
#include "../../include/ured_hip.h"

namespace {

typedef unsigned long long u64;
typedef unsigned int u32;

constexpr int GP_NMAX = URED_FPS_NMAX;   // 16384 = 1024 threads x 16 points
constexpr int GP_TMAX = 1024;
constexpr int GP_WMAX = GP_TMAX / 64;

__device__ __forceinline__ float gp_sqd(float px, float py, float pz, float cx, float cy, float cz) {
    const float dx = px - cx, dy = py - cy, dz = pz - cz;
    return ((dx * dx) + (dy * dy)) + (dz * dz);
}

struct FpsSlot { u64 key; float x, y, z, pad; };

template <int PPT>
__global__ __launch_bounds__(GP_TMAX) void fps_kernel(const float* __restrict__ xyz, const int* __restrict__ start,
                                                      int N, int npoint, int* __restrict__ idx_out) {
    __shared__ FpsSlot slot[2][GP_WMAX];
    const int b = blockIdx.x, t = threadIdx.x, T = blockDim.x, W = T >> 6, wv = t >> 6;
    const float* X = xyz + (size_t)b * N * 3;
    int* out = idx_out + (size_t)b * npoint;
    float px[PPT], py[PPT], pz[PPT], dm[PPT];
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
        const int j = t + k * T;
        const bool in = j < N;
        px[k] = in ? X[3 * (size_t)j] : 0.f;
        py[k] = in ? X[3 * (size_t)j + 1] : 0.f;
        pz[k] = in ? X[3 * (size_t)j + 2] : 0.f;
        dm[k] = in ? 1e10f : 0.f;
    }
    int f = min(max(start[b], 0), N - 1);             // any start is defined: clamped
    float cx = X[3 * (size_t)f], cy = X[3 * (size_t)f + 1], cz = X[3 * (size_t)f + 2];
    int buf = 0;
    for (int i = 0;; ++i) {
        if (t == 0) {
            URED_DBG_CHECK(i < npoint && f >= 0 && f < N);
            out[i] = f;
        }
        if (i == npoint - 1) break;
        u64 best = 0;
        float bx = 0.f, by = 0.f, bz = 0.f;
#pragma unroll
        for (int k = 0; k < PPT; ++k) {
            const float d = gp_sqd(px[k], py[k], pz[k], cx, cy, cz);
            dm[k] = d < dm[k] ? d : dm[k];
            const u64 key = ((u64)__float_as_uint(dm[k]) << 32) | (u32)~(u32)(t + k * T);
            const bool up = key > best;
            best = up ? key : best;
            bx = up ? px[k] : bx; by = up ? py[k] : by; bz = up ? pz[k] : bz;
        }
        u64 m = best;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const u64 v = __shfl_xor(m, o);
            m = v > m ? v : m;
        }
        if (m == best) {                              // keys are unique: exactly one lane of the wave
            FpsSlot& s = slot[buf][wv];
            s.key = m; s.x = bx; s.y = by; s.z = bz;
        }
        __syncthreads();
        u64 g = slot[buf][0].key;
        int gw = 0;
        for (int w = 1; w < W; ++w) {
            const u64 v = slot[buf][w].key;
            const bool up = v > g;
            g = up ? v : g;
            gw = up ? w : gw;
        }
        f = (int)~(u32)g;
        URED_DBG_CHECK(f >= 0 && f < N);
        cx = slot[buf][gw].x; cy = slot[buf][gw].y; cz = slot[buf][gw].z;
        buf ^= 1;
    }
}

constexpr int BQ_T = 256;   // 4 queries per workgroup

__global__ __launch_bounds__(BQ_T) void ball_query_kernel(const float* __restrict__ xyz, const float* __restrict__ new_xyz,
                                                          int N, int S, float r2, int nsample, int* __restrict__ idx_out) {
    const int b = blockIdx.y, ln = threadIdx.x & 63;
    const int s = blockIdx.x * (BQ_T / 64) + (threadIdx.x >> 6);
    if (s >= S) return;                               // wave-uniform
    const float* X = xyz + (size_t)b * N * 3;
    const float* q = new_xyz + ((size_t)b * S + s) * 3;
    const float qx = q[0], qy = q[1], qz = q[2];
    int* row = idx_out + ((size_t)b * S + s) * nsample;
    int cnt = 0, first = N;
    for (int j0 = 0; j0 < N && cnt < nsample; j0 += 64) {
        const int j = j0 + ln;
        bool hit = false;
        if (j < N) {
            const float d = gp_sqd(X[3 * (size_t)j], X[3 * (size_t)j + 1], X[3 * (size_t)j + 2], qx, qy, qz);
            hit = !(d > r2);
        }
        const u64 mask = __ballot(hit);
        if (mask == 0) continue;
        if (cnt == 0) first = j0 + (int)__builtin_ctzll(mask);
        const int pos = cnt + (int)__popcll(mask & ((1ull << ln) - 1ull));
        if (hit && pos < nsample) {
            URED_DBG_CHECK(pos >= 0 && j < N);
            row[pos] = j;
        }
        cnt += (int)__popcll(mask);
    }
    for (int p = min(cnt, nsample) + ln; p < nsample; p += 64) row[p] = first;   // padding; N when empty
}

constexpr int GF_T = 256;

// out[(b,s,k), :] = [xyz[b,idx] - new_xyz[b,s] (when xyz is given), points[b,idx]]; zero row for idx outside [0,N)
__global__ __launch_bounds__(GF_T) void group_fwd_kernel(const float* __restrict__ xyz, const float* __restrict__ new_xyz,
                                                         const float* __restrict__ points, const int* __restrict__ idx,
                                                         int N, int S, int K, int D, int C3, u32 total,
                                                         float* __restrict__ out) {
    const u32 e = blockIdx.x * (u32)GF_T + threadIdx.x;   // B * S * K * C < 2^31 (host check)
    if (e >= total) return;
    const u32 C = (u32)(C3 + D);
    const u32 r = e / C;
    const int c = (int)(e - r * C);
    const u32 bs = r / (u32)K;                        // b * S + s
    const u32 b = bs / (u32)S;
    const int id = idx[r];
    URED_DBG_CHECK(id >= 0 && id <= N);               // N is the ball query's empty-row value
    float v = 0.f;
    if ((u32)id < (u32)N) {
        const size_t p = (size_t)b * N + id;
        if (c < C3) v = xyz[3 * p + c] - new_xyz[3 * (size_t)bs + c];
        else v = points[p * D + (c - C3)];
    }
    out[e] = v;
}

constexpr int GB_P = 32, GB_C = 64;                   // points x channels of one wave
constexpr int GB_U = 4;                               // loads kept in flight: index batches, and g rows

__global__ __launch_bounds__(64) void group_bwd_kernel(const float* __restrict__ g, const int* __restrict__ idx, int N,
                                                       int E, int D, int C3, float* __restrict__ grad_xyz,
                                                       float* __restrict__ grad_points) {
    __shared__ float acc[GB_P * GB_C];                // column ln belongs to lane ln alone: no barrier anywhere
    const int ln = threadIdx.x, b = blockIdx.z, j0 = blockIdx.x * GB_P, c = blockIdx.y * GB_C + ln;
    const int C = C3 + D;
    const bool cin = c < C;
    const int* I = idx + (size_t)b * E;
    const float* G = g + (size_t)b * E * C + (cin ? c : 0);
#pragma unroll
    for (int p = 0; p < GB_P; ++p) acc[p * GB_C + ln] = 0.f;
    for (int e0 = 0; e0 < E; e0 += 64 * GB_U) {
        int pl[GB_U];
#pragma unroll
        for (int u = 0; u < GB_U; ++u) {              // GB_U batches of 64 indices, loaded together
            const int e = e0 + 64 * u + ln;
            const int id = e < E ? I[e] : -1;
            URED_DBG_CHECK(e >= E || (id >= 0 && id <= N));
            pl[u] = id < N ? id - j0 : -1;
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
                    v[q] = (l[q] >= 0 && cin) ? G[(size_t)(eb + l[q]) * C] : 0.f;
                }
#pragma unroll
                for (int q = 0; q < GB_U; ++q) {
                    if (l[q] < 0) break;              // wave-uniform
                    const int p = __builtin_amdgcn_readlane(pl[u], l[q]);
                    URED_DBG_CHECK(p >= 0 && p < GB_P);
                    acc[p * GB_C + ln] += v[q];
                }
            }
        }
    }
    if (!cin) return;
    for (int p = 0; p < GB_P; ++p) {
        const int j = j0 + p;
        if (j >= N) break;
        const size_t pt = (size_t)b * N + j;
        const float v = acc[p * GB_C + ln];
        if (c < C3) grad_xyz[3 * pt + c] = v;
        else grad_points[pt * D + (c - C3)] = v;
    }
}

// grad_new_xyz[b,s,c] = - sum_k g[(b,s,k), c] over the rows whose index lies in [0,N), k ascending
__global__ __launch_bounds__(GF_T) void group_bwd_center_kernel(const float* __restrict__ g, const int* __restrict__ idx,
                                                                int N, int K, int C, long long total,
                                                                float* __restrict__ grad_new_xyz) {
    const long long t = (long long)blockIdx.x * GF_T + threadIdx.x;
    if (t >= total) return;
    const long long bs = t / 3;
    const int c = (int)(t - bs * 3);
    float a = 0.f;
    for (int k = 0; k < K; ++k) {
        const long long r = bs * K + k;
        const int id = idx[r];
        URED_DBG_CHECK(id >= 0 && id <= N);
        if ((u32)id < (u32)N) a += g[r * C + c];
    }
    grad_new_xyz[t] = -a;
}

int group_check(const char* who, int B, int N, int S, int K, int D) {
    URED_REQUIRE(B >= 0 && S >= 0 && D >= 0, "%s: negative size (B=%d S=%d D=%d)", who, B, S, D);
    URED_REQUIRE(N >= 1 && K >= 1, "%s: N %d and K %d must be at least 1", who, N, K);
    URED_REQUIRE(B <= 65535, "%s: B %d exceeds 65535", who, B);
    URED_REQUIRE((long long)B * N * (D > 3 ? D : 3) < (1ll << 31), "%s: B * N * max(D, 3) = %lld exceeds 2^31 - 1", who,
                 (long long)B * N * (D > 3 ? D : 3));
    URED_REQUIRE((long long)B * S * K * (3 + D) < (1ll << 31), "%s: B * S * K * (3 + D) = %lld exceeds 2^31 - 1", who,
                 (long long)B * S * K * (3 + D));
    return 0;
}

}  // namespace

extern "C" {

int ured_fps(const float* xyz, const int* start, int B, int N, int npoint, int* idx_out, void* stream) {
    ured::clear_error();
    URED_REQUIRE(B >= 0, "ured_fps: negative size (B %d)", B);
    URED_REQUIRE(N >= 1 && N <= GP_NMAX, "ured_fps: N %d outside [1, %d]", N, GP_NMAX);
    URED_REQUIRE(npoint >= 1, "ured_fps: npoint %d must be at least 1", npoint);
    URED_REQUIRE(B <= 65535, "ured_fps: B %d exceeds 65535", B);
    URED_REQUIRE((long long)B * npoint < (1ll << 31), "ured_fps: B * npoint = %lld exceeds 2^31 - 1", (long long)B * npoint);
    if (B == 0) return 0;
    URED_REQUIRE(xyz && start && idx_out, "ured_fps: null pointer");
    // four points per thread up to 1024 threads, then more points per thread
    int T = 64;
    while (T < GP_TMAX && T * 4 < N) T <<= 1;
    const int ppt = (N + T - 1) / T;
    hipStream_t st = (hipStream_t)stream;
#define URED_FPS_LAUNCH(P) hipLaunchKernelGGL(fps_kernel<P>, dim3(B), dim3(T), 0, st, xyz, start, N, npoint, idx_out)
    if (ppt <= 1) URED_FPS_LAUNCH(1);
    else if (ppt <= 2) URED_FPS_LAUNCH(2);
    else if (ppt <= 4) URED_FPS_LAUNCH(4);
    else if (ppt <= 8) URED_FPS_LAUNCH(8);
    else URED_FPS_LAUNCH(16);
#undef URED_FPS_LAUNCH
    return ured::launch_status("ured_fps");
}

int ured_ball_query(const float* xyz, const float* new_xyz, int B, int N, int S, float r2, int nsample, int* idx_out,
                    void* stream) {
    ured::clear_error();
    if (const int rc = group_check("ured_ball_query", B, N, S, nsample, 0)) return rc;
    URED_REQUIRE(!(r2 < 0.f), "ured_ball_query: r2 %g is negative", (double)r2);
    if (B == 0 || S == 0) return 0;
    URED_REQUIRE(xyz && new_xyz && idx_out, "ured_ball_query: null pointer");
    hipLaunchKernelGGL(ball_query_kernel, dim3((S + BQ_T / 64 - 1) / (BQ_T / 64), B), dim3(BQ_T), 0, (hipStream_t)stream,
                       xyz, new_xyz, N, S, r2, nsample, idx_out);
    return ured::launch_status("ured_ball_query");
}

int ured_group_fwd(const float* xyz, const float* new_xyz, const float* points, const int* idx, int B, int N, int S,
                   int K, int D, float* out, void* stream) {
    ured::clear_error();
    if (const int rc = group_check("ured_group_fwd", B, N, S, K, D)) return rc;
    URED_REQUIRE((xyz == nullptr) == (new_xyz == nullptr), "ured_group_fwd: xyz and new_xyz go together");
    URED_REQUIRE((points != nullptr) == (D > 0), "ured_group_fwd: points and D > 0 go together (D %d)", D);
    const int C3 = xyz ? 3 : 0;
    URED_REQUIRE(C3 + D > 0, "ured_group_fwd: nothing to gather (no xyz, D 0)");
    if (B == 0 || S == 0) return 0;
    URED_REQUIRE(idx && out, "ured_group_fwd: null pointer");
    const long long total = (long long)B * S * K * (C3 + D);
    hipLaunchKernelGGL(group_fwd_kernel, dim3((unsigned)((total + GF_T - 1) / GF_T)), dim3(GF_T), 0, (hipStream_t)stream,
                       xyz, new_xyz, points, idx, N, S, K, D, C3, (u32)total, out);
    return ured::launch_status("ured_group_fwd");
}

int ured_group_bwd(const float* grad_out, const int* idx, int B, int N, int S, int K, int D, float* grad_xyz,
                   float* grad_new_xyz, float* grad_points, void* stream) {
    ured::clear_error();
    if (const int rc = group_check("ured_group_bwd", B, N, S, K, D)) return rc;
    URED_REQUIRE((grad_xyz == nullptr) == (grad_new_xyz == nullptr), "ured_group_bwd: grad_xyz and grad_new_xyz go together");
    URED_REQUIRE((grad_points != nullptr) == (D > 0), "ured_group_bwd: grad_points and D > 0 go together (D %d)", D);
    const int C3 = grad_xyz ? 3 : 0;
    URED_REQUIRE(C3 + D > 0, "ured_group_bwd: nothing to scatter (no grad_xyz, D 0)");
    URED_REQUIRE((long long)S * K < (1ll << 31), "ured_group_bwd: S * K = %lld exceeds 2^31 - 1", (long long)S * K);
    if (B == 0) return 0;
    URED_REQUIRE(S == 0 || (grad_out && idx), "ured_group_bwd: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const int C = C3 + D;
    hipLaunchKernelGGL(group_bwd_kernel, dim3((N + GB_P - 1) / GB_P, (C + GB_C - 1) / GB_C, B), dim3(64), 0, st, grad_out,
                       idx, N, S * K, D, C3, grad_xyz, grad_points);
    if (C3 && S > 0) {
        const long long total = (long long)B * S * 3;
        hipLaunchKernelGGL(group_bwd_center_kernel, dim3((unsigned)((total + GF_T - 1) / GF_T)), dim3(GF_T), 0, st, grad_out,
                           idx, N, K, C, total, grad_new_xyz);
    }
    return ured::launch_status("ured_group_bwd");
}

}  // extern "C"

URED_DBG_ACCESSOR(ured_dbg_group)
