// gcn.hip — 3D-GCN graph convolution (the reference's network/P_3DGC.py: Conv_surface, Conv_layer,
// Pool_layer) without the [B, V, n, S*C] tensors that the torch composition builds and keeps.
// Plain pointers, the caller's stream, no allocation, no host sync, no device state, no float
// atomics; every limit is checked on the host before any device work. Activations are point-major
// fp32 rows [B*V, .]; indices are int32 and local to their cloud. An index outside [0, V) reads as
// a zero row (a zero direction in ured_gcn_dirs) and takes no gradient.
//
// Arithmetic contract (the file is built with -ffp-contract=off and spells the order out):
//   theta(v, j, s, c) = max(((d.x * a.x) + (d.y * a.y)) + (d.z * a.z), 0),
//       d = dirn[b, v, j, :], a = sdn[:, s*C + c]
//   prod = theta * feat[b, idx[b,v,j], C + s*C + c]      (layer form; surface form: prod = theta)
//   m_s  = max_j prod, the lowest j winning a tie (strict > against the running maximum, slot 0 first)
//   out  = feat[b, v, c] + ((m_0 + m_1) + ... + m_{S-1})  (surface form: without the centre term)
//
// ured_gcn_dirs.  One thread per (b, v, j).
//
// ured_gcn_conv_fwd.  Lanes across 64 channels, one wave per vertex, four vertices per pass of a
// 256-thread workgroup, GC_VT vertices per workgroup. The lane's S support directions (3 * S
// floats) sit in registers for all of them; a vertex's n indices and n x 3 directions are
// wave-uniform loads; each neighbour costs S coalesced 256-byte reads of its feature row.
//
// ured_gcn_conv_bwd, three launches.
//   grad_sdn: the forward's tiling walked again. Per (v, s, c) the winning slot j* gives the
//     direction and the feature value back (a per-lane read of at most n distinct rows);
//     g * f * d[j*] is added to the lane's 3 * S register sums when theta > 0. The four waves of a
//     workgroup combine through LDS in wave order, the workgroup stores one partial row, and a second
//     kernel adds the partial rows in ascending order: fixed order throughout.
//   grad_feat: the idiom of group.hip's group_bwd_kernel. One wave per (32 target rows, 64 columns of
//     the (S+1)*C) of a cloud scans the cloud's V * n indices in ascending (v, j) order, 64 at a time,
//     picks the entries that land in its rows (a ballot, walked from its lowest bit) and for each,
//     in order, the lanes whose slot is j add g[v, c] * theta to the row's accumulator in LDS. Centre
//     columns copy g. Every element is written once; a second run is bitwise equal.
//
// ured_gcn_pool_fwd / _bwd.  max_j feat[b, idx[b, sample[p], j], c] with its slot, one thread per
// output element; the backward is the same scan over the cloud's P * k entries.
#include <hip/hip_runtime.h>
#define URED_DBG_FILE 14
#include "ured_common.h"
#include "../../include/ured_hip.h"

namespace {

typedef unsigned long long u64;
typedef unsigned int u32;
typedef unsigned char u8;

constexpr int GC_T = 256;                   // 4 waves: 4 vertices per pass
constexpr int GC_W = GC_T / 64;
constexpr int GC_VT = 16;                   // vertices per workgroup of the forward
constexpr int GC_SMAX = URED_GCN_SMAX;
constexpr int GC_P = 32, GC_C = 64;         // target rows x columns of one scatter wave

__device__ __forceinline__ float gc_theta(float dx, float dy, float dz, float ax, float ay, float az) {
    const float t = ((dx * ax) + (dy * ay)) + (dz * az);
    return t > 0.f ? t : 0.f;
}

__global__ __launch_bounds__(GC_T) void gcn_dirs_kernel(const float* __restrict__ xyz, const int* __restrict__ idx, int V,
                                                        int n, u32 total, float* __restrict__ out) {
    const u32 e = blockIdx.x * (u32)GC_T + threadIdx.x;      // B * V * n * 3 < 2^31 (host check)
    if (e >= total) return;
    const u32 row = e / (u32)n;                              // b * V + v
    const u32 b = row / (u32)V;
    const int id = idx[e];
    float ox = 0.f, oy = 0.f, oz = 0.f;
    if ((u32)id < (u32)V) {
        const float* p = xyz + 3 * ((size_t)b * V + id);
        const float* c = xyz + 3 * (size_t)row;
        const float dx = p[0] - c[0], dy = p[1] - c[1], dz = p[2] - c[2];
        const float nrm = __fsqrt_rn(((dx * dx) + (dy * dy)) + (dz * dz));
        const float den = nrm > 1e-12f ? nrm : 1e-12f;
        ox = __fdiv_rn(dx, den); oy = __fdiv_rn(dy, den); oz = __fdiv_rn(dz, den);
    }
    out[3 * (size_t)e] = ox; out[3 * (size_t)e + 1] = oy; out[3 * (size_t)e + 2] = oz;
}

// feat == nullptr: the surface form. LD = (S + 1) * C is feat's row length.
template <int S>
__global__ __launch_bounds__(GC_T) void gcn_conv_fwd_kernel(const float* __restrict__ dirn, const float* __restrict__ sdn,
                                                            const float* __restrict__ feat, const int* __restrict__ idx,
                                                            int BV, int V, int n, int C, float* __restrict__ out,
                                                            u8* __restrict__ slot) {
    const int ln = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int c = blockIdx.y * 64 + ln;
    const bool cin = c < C;
    const int cc = cin ? c : 0;
    const int SC = S * C, LD = SC + C;
    float ax[S], ay[S], az[S];
#pragma unroll
    for (int s = 0; s < S; ++s) {
        ax[s] = sdn[s * C + cc]; ay[s] = sdn[SC + s * C + cc]; az[s] = sdn[2 * SC + s * C + cc];
    }
    const int r0 = blockIdx.x * GC_VT;
    for (int t = wv; t < GC_VT; t += GC_W) {
        const int row = __builtin_amdgcn_readfirstlane(r0 + t);
        if (row >= BV) break;                                // wave-uniform
        const size_t base = (size_t)(row / V) * V;           // first row of the cloud
        const int* I = idx + (size_t)row * n;
        const float* D = dirn + (size_t)row * n * 3;
        float best[S];
        int bj[S];
#pragma unroll
        for (int s = 0; s < S; ++s) { best[s] = 0.f; bj[s] = 0; }
        for (int j = 0; j < n; ++j) {
            const int id = __builtin_amdgcn_readfirstlane(I[j]);
            const float dx = D[3 * j], dy = D[3 * j + 1], dz = D[3 * j + 2];
            const bool ok = (u32)id < (u32)V;
            const float* F = feat ? feat + (base + (ok ? id : 0)) * (size_t)LD + C + cc : nullptr;
            float f[S];
#pragma unroll
            for (int s = 0; s < S; ++s) f[s] = feat ? (ok ? F[s * C] : 0.f) : 1.f;
#pragma unroll
            for (int s = 0; s < S; ++s) {
                const float p = gc_theta(dx, dy, dz, ax[s], ay[s], az[s]) * f[s];
                const bool up = j == 0 || p > best[s];
                best[s] = up ? p : best[s];
                bj[s] = up ? j : bj[s];
            }
        }
        if (!cin) continue;
        float acc = best[0];
#pragma unroll
        for (int s = 1; s < S; ++s) acc += best[s];
        URED_DBG_CHECK(row >= 0 && row < BV && c < C);
        out[(size_t)row * C + c] = feat ? feat[(size_t)row * LD + c] + acc : acc;
#pragma unroll
        for (int s = 0; s < S; ++s) slot[((size_t)row * S + s) * C + c] = (u8)bj[s];
    }
}

// Partial sums of grad_sdn: workgroup (x, y) covers the rows_per_block vertices from x * rows_per_block
// (wave w takes every fourth from w) and the channels of chunk y; ws[x][k][s*C + c], k = 0..2.
template <int S>
__global__ __launch_bounds__(GC_T) void gcn_conv_bwd_sdn_kernel(const float* __restrict__ g, const float* __restrict__ dirn,
                                                                const float* __restrict__ sdn, const float* __restrict__ feat,
                                                                const int* __restrict__ idx, const u8* __restrict__ slot,
                                                                int BV, int V, int n, int C, int rows_per_block,
                                                                float* __restrict__ ws) {
    __shared__ float part[GC_W][3 * S][64];
    const int ln = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int c = blockIdx.y * 64 + ln;
    const bool cin = c < C;
    const int cc = cin ? c : 0;
    const int SC = S * C, LD = SC + C;
    float ax[S], ay[S], az[S], sx[S], sy[S], sz[S];
#pragma unroll
    for (int s = 0; s < S; ++s) {
        ax[s] = sdn[s * C + cc]; ay[s] = sdn[SC + s * C + cc]; az[s] = sdn[2 * SC + s * C + cc];
        sx[s] = sy[s] = sz[s] = 0.f;
    }
    const int r0 = blockIdx.x * rows_per_block;
    for (int t = wv; t < rows_per_block; t += GC_W) {
        const int row = __builtin_amdgcn_readfirstlane(r0 + t);
        if (row >= BV) break;                                // wave-uniform
        if (!cin) continue;
        const size_t base = (size_t)(row / V) * V;
        const int* I = idx + (size_t)row * n;
        const float* D = dirn + (size_t)row * n * 3;
        const float gv = g[(size_t)row * C + c];
#pragma unroll
        for (int s = 0; s < S; ++s) {
            const int j = slot[((size_t)row * S + s) * C + c];
            URED_DBG_CHECK(j < n);
            const int jj = j < n ? j : 0;
            const float dx = D[3 * jj], dy = D[3 * jj + 1], dz = D[3 * jj + 2];
            const float th = gc_theta(dx, dy, dz, ax[s], ay[s], az[s]);
            float f = 1.f;
            if (feat) {
                const int id = I[jj];
                f = (u32)id < (u32)V ? feat[(base + id) * (size_t)LD + C + s * C + c] : 0.f;
            }
            if (th > 0.f) {                                  // relu passes a gradient iff theta > 0
                const float w = gv * f;
                sx[s] += w * dx; sy[s] += w * dy; sz[s] += w * dz;
            }
        }
    }
#pragma unroll
    for (int s = 0; s < S; ++s) {
        part[wv][3 * s][ln] = sx[s]; part[wv][3 * s + 1][ln] = sy[s]; part[wv][3 * s + 2][ln] = sz[s];
    }
    __syncthreads();
    if (wv != 0 || !cin) return;
    float* W = ws + (size_t)blockIdx.x * 3 * SC;
#pragma unroll
    for (int s = 0; s < S; ++s) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            float a = part[0][3 * s + k][ln];
#pragma unroll
            for (int w = 1; w < GC_W; ++w) a += part[w][3 * s + k][ln];
            W[k * SC + s * C + c] = a;
        }
    }
}

// out[e] = ws[0][e] + ws[1][e] + ... in ascending order
__global__ __launch_bounds__(GC_T) void gcn_partial_sum_kernel(const float* __restrict__ ws, int nparts, int len,
                                                               float* __restrict__ out) {
    const int e = blockIdx.x * GC_T + threadIdx.x;
    if (e >= len) return;
    float a = 0.f;
    for (int p = 0; p < nparts; ++p) a += ws[(size_t)p * len + e];
    out[e] = a;
}

// The scan of group_bwd_kernel: entries e = 0..E-1 of cloud b in ascending order, target(e) its row in
// [0, V) (or outside: skipped); add(e, p) adds entry e's term to LDS row p of the lane's column.
template <class Target, class Add>
__device__ __forceinline__ void gc_scan(int E, int V, int j0, int ln, Target target, Add add) {
    for (int e0 = 0; e0 < E; e0 += 64) {
        const int e = e0 + ln;
        const int id = e < E ? target(e) : -1;
        const int pl = (u32)id < (u32)V ? id - j0 : -1;
        u64 mask = __ballot((u32)pl < (u32)GC_P);
        while (mask) {                                       // the wave's entries of this batch, ascending
            const int l = (int)__builtin_ctzll(mask);
            mask &= mask - 1;
            const int p = __builtin_amdgcn_readlane(pl, l);
            URED_DBG_CHECK(p >= 0 && p < GC_P && e0 + l < E);
            add(e0 + l, p);
        }
    }
}

__global__ __launch_bounds__(64) void gcn_conv_bwd_feat_kernel(const float* __restrict__ g, const float* __restrict__ dirn,
                                                               const float* __restrict__ sdn, const int* __restrict__ idx,
                                                               const u8* __restrict__ slot, int V, int n, int S, int C,
                                                               float* __restrict__ grad_feat) {
    __shared__ float acc[GC_P * GC_C];                       // column ln belongs to lane ln alone: no barrier anywhere
    const int ln = threadIdx.x, b = blockIdx.z, j0 = blockIdx.x * GC_P, col = blockIdx.y * GC_C + ln;
    const int SC = S * C, LD = SC + C;
    const bool centre = col < C, sup = col >= C && col < LD;
    const int sc = sup ? col - C : 0;                        // s * C + c
    const int s = sc / C, c = centre ? col : sc - s * C;
    const float ax = sdn[sc], ay = sdn[SC + sc], az = sdn[2 * SC + sc];
    const size_t base = (size_t)b * V;
    const int* I = idx + base * n;
#pragma unroll
    for (int p = 0; p < GC_P; ++p) acc[p * GC_C + ln] = 0.f;
    gc_scan(V * n, V, j0, ln, [&](int e) { return I[e]; }, [&](int e, int p) {
        const int v = e / n, j = e - v * n;                  // wave-uniform
        const size_t row = base + v;
        if (sup && slot[(row * S + s) * C + c] == (u8)j) {
            const float* D = dirn + (row * n + j) * 3;
            acc[p * GC_C + ln] += g[row * C + c] * gc_theta(D[0], D[1], D[2], ax, ay, az);
        }
    });
    if (!centre && !sup) return;
    for (int p = 0; p < GC_P; ++p) {
        const int r = j0 + p;
        if (r >= V) break;
        grad_feat[(base + r) * LD + col] = centre ? g[(base + r) * C + c] : acc[p * GC_C + ln];
    }
}

__global__ __launch_bounds__(GC_T) void gcn_pool_fwd_kernel(const float* __restrict__ feat, const int* __restrict__ idx,
                                                            const int* __restrict__ sample, int V, int k, int P, int C,
                                                            u32 total, float* __restrict__ out, u8* __restrict__ slot) {
    const u32 e = blockIdx.x * (u32)GC_T + threadIdx.x;      // B * P * C < 2^31 (host check)
    if (e >= total) return;
    const u32 r = e / (u32)C;                                // b * P + p
    const int c = (int)(e - r * (u32)C);
    const u32 b = r / (u32)P;
    const int sv = sample[r - b * (u32)P];
    float best = 0.f;
    int bj = 0;
    if ((u32)sv < (u32)V) {
        const int* I = idx + ((size_t)b * V + sv) * k;
        for (int j = 0; j < k; ++j) {
            const int id = I[j];
            const float v = (u32)id < (u32)V ? feat[((size_t)b * V + id) * C + c] : 0.f;
            const bool up = j == 0 || v > best;
            best = up ? v : best;
            bj = up ? j : bj;
        }
    }
    out[e] = best;
    slot[e] = (u8)bj;
}

__global__ __launch_bounds__(64) void gcn_pool_bwd_kernel(const float* __restrict__ g, const int* __restrict__ idx,
                                                          const int* __restrict__ sample, const u8* __restrict__ slot,
                                                          int V, int k, int P, int C, float* __restrict__ grad_feat) {
    __shared__ float acc[GC_P * GC_C];
    const int ln = threadIdx.x, b = blockIdx.z, j0 = blockIdx.x * GC_P, c = blockIdx.y * GC_C + ln;
    const bool cin = c < C;
    const size_t base = (size_t)b * V;
#pragma unroll
    for (int p = 0; p < GC_P; ++p) acc[p * GC_C + ln] = 0.f;
    gc_scan(P * k, V, j0, ln, [&](int e) {
        const int q = e / k, sv = sample[q];
        return (u32)sv < (u32)V ? idx[(base + sv) * k + (e - q * k)] : -1;
    }, [&](int e, int p) {
        const int q = e / k, j = e - q * k;                  // wave-uniform
        const size_t r = ((size_t)b * P + q) * C + c;
        if (cin && slot[r] == (u8)j) acc[p * GC_C + ln] += g[r];
    });
    if (!cin) return;
    for (int p = 0; p < GC_P; ++p) {
        const int r = j0 + p;
        if (r >= V) break;
        grad_feat[(base + r) * C + c] = acc[p * GC_C + ln];
    }
}

int gcn_check(const char* who, int B, int V, int n, int S, int C) {
    URED_REQUIRE(B >= 0, "%s: negative size (B %d)", who, B);
    URED_REQUIRE(V >= 1 && C >= 1, "%s: V %d and C %d must be at least 1", who, V, C);
    URED_REQUIRE(n >= 1 && n <= URED_GCN_NMAX, "%s: n %d outside [1, %d] (the winning slot is a uint8)", who, n,
                 URED_GCN_NMAX);
    URED_REQUIRE(S >= 1 && S <= GC_SMAX, "%s: S %d outside [1, %d] (the supports live in registers)", who, S, GC_SMAX);
    URED_REQUIRE(B <= 65535, "%s: B %d exceeds 65535", who, B);
    URED_REQUIRE((long long)B * V * (S + 1) * C < (1ll << 31), "%s: B * V * (S + 1) * C = %lld exceeds 2^31 - 1", who,
                 (long long)B * V * (S + 1) * C);
    URED_REQUIRE((long long)B * V * n * 3 < (1ll << 31), "%s: B * V * n * 3 = %lld exceeds 2^31 - 1", who,
                 (long long)B * V * n * 3);
    return 0;
}

int pool_check(const char* who, int B, int V, int k, int P, int C) {
    URED_REQUIRE(B >= 0 && P >= 0, "%s: negative size (B %d P %d)", who, B, P);
    URED_REQUIRE(V >= 1 && C >= 1, "%s: V %d and C %d must be at least 1", who, V, C);
    URED_REQUIRE(k >= 1 && k <= URED_GCN_NMAX, "%s: k %d outside [1, %d] (the winning slot is a uint8)", who, k,
                 URED_GCN_NMAX);
    URED_REQUIRE(B <= 65535, "%s: B %d exceeds 65535", who, B);
    URED_REQUIRE((long long)B * V * C < (1ll << 31) && (long long)B * P * C < (1ll << 31),
                 "%s: B * V * C and B * P * C must stay below 2^31 (B=%d V=%d P=%d C=%d)", who, B, V, P, C);
    URED_REQUIRE((long long)B * V * k < (1ll << 31) && (long long)P * k < (1ll << 31),
                 "%s: B * V * k and P * k must stay below 2^31 (B=%d V=%d P=%d k=%d)", who, B, V, P, k);
    return 0;
}

}  // namespace

extern "C" {

int ured_gcn_dirs(const float* vertices, const int* idx, int B, int V, int n, float* out, void* stream) {
    ured::clear_error();
    if (const int rc = gcn_check("ured_gcn_dirs", B, V, n, 1, 1)) return rc;
    if (B == 0) return 0;
    URED_REQUIRE(vertices && idx && out, "ured_gcn_dirs: null pointer");
    const long long total = (long long)B * V * n;
    hipLaunchKernelGGL(gcn_dirs_kernel, dim3((unsigned)((total + GC_T - 1) / GC_T)), dim3(GC_T), 0, (hipStream_t)stream,
                       vertices, idx, V, n, (u32)total, out);
    return ured::launch_status("ured_gcn_dirs");
}

#define URED_GCN_BY_S(LAUNCH)                                                   \
    switch (S) {                                                                \
        case 1: LAUNCH(1); break; case 2: LAUNCH(2); break; case 3: LAUNCH(3); break; case 4: LAUNCH(4); break; \
        case 5: LAUNCH(5); break; case 6: LAUNCH(6); break; case 7: LAUNCH(7); break; default: LAUNCH(8); break; \
    }

int ured_gcn_conv_fwd(const float* dirn, const float* sdn, const float* feat, const int* idx, int B, int V, int n, int S,
                      int C, float* out, unsigned char* slot, void* stream) {
    ured::clear_error();
    if (const int rc = gcn_check("ured_gcn_conv_fwd", B, V, n, S, C)) return rc;
    if (B == 0) return 0;
    URED_REQUIRE(dirn && sdn && idx && out && slot, "ured_gcn_conv_fwd: null pointer");
    const int BV = B * V;
    const dim3 grid((BV + GC_VT - 1) / GC_VT, (C + 63) / 64);
    hipStream_t st = (hipStream_t)stream;
#define URED_GCN_FWD(SS) hipLaunchKernelGGL(gcn_conv_fwd_kernel<SS>, grid, dim3(GC_T), 0, st, dirn, sdn, feat, idx, BV, V, n, C, out, slot)
    URED_GCN_BY_S(URED_GCN_FWD)
#undef URED_GCN_FWD
    return ured::launch_status("ured_gcn_conv_fwd");
}

int ured_gcn_conv_bwd_parts(int B, int V) {
    const long long BV = (long long)(B > 0 ? B : 0) * (V > 0 ? V : 0);
    const long long by_rows = (BV + URED_GCN_BWD_ROWS - 1) / URED_GCN_BWD_ROWS;
    return (int)(by_rows < URED_GCN_BWD_PARTS ? (by_rows > 0 ? by_rows : 1) : URED_GCN_BWD_PARTS);
}

int ured_gcn_conv_bwd(const float* grad_out, const float* dirn, const float* sdn, const float* feat, const int* idx,
                      const unsigned char* slot, int B, int V, int n, int S, int C, float* grad_feat, float* grad_sdn,
                      float* ws, size_t ws_floats, void* stream) {
    ured::clear_error();
    if (const int rc = gcn_check("ured_gcn_conv_bwd", B, V, n, S, C)) return rc;
    URED_REQUIRE((feat != nullptr) == (grad_feat != nullptr), "ured_gcn_conv_bwd: feat and grad_feat go together");
    URED_REQUIRE((long long)V * n < (1ll << 31), "ured_gcn_conv_bwd: V * n = %lld exceeds 2^31 - 1", (long long)V * n);
    const int parts = ured_gcn_conv_bwd_parts(B, V);
    const size_t need = (size_t)parts * 3 * S * C;
    URED_REQUIRE(ws_floats >= need, "ured_gcn_conv_bwd: workspace of %zu floats, %zu needed", ws_floats, need);
    URED_REQUIRE(grad_sdn, "ured_gcn_conv_bwd: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const int len = 3 * S * C;
    if (B == 0) {                                            // the sum over no vertices
        if (hipMemsetAsync(grad_sdn, 0, sizeof(float) * len, st) != hipSuccess) return ured::launch_status("ured_gcn_conv_bwd");
        return 0;
    }
    URED_REQUIRE(grad_out && dirn && sdn && idx && slot && ws, "ured_gcn_conv_bwd: null pointer");
    const int BV = B * V;
    const int rows = (BV + parts - 1) / parts;               // vertices per workgroup; parts * rows >= BV
    const dim3 grid(parts, (C + 63) / 64);
#define URED_GCN_BWD(SS) hipLaunchKernelGGL(gcn_conv_bwd_sdn_kernel<SS>, grid, dim3(GC_T), 0, st, grad_out, dirn, sdn, feat, idx, slot, BV, V, n, C, rows, ws)
    URED_GCN_BY_S(URED_GCN_BWD)
#undef URED_GCN_BWD
    hipLaunchKernelGGL(gcn_partial_sum_kernel, dim3((len + GC_T - 1) / GC_T), dim3(GC_T), 0, st, ws, parts, len, grad_sdn);
    if (feat) {
        const int LD = (S + 1) * C;
        hipLaunchKernelGGL(gcn_conv_bwd_feat_kernel, dim3((V + GC_P - 1) / GC_P, (LD + GC_C - 1) / GC_C, B), dim3(64), 0, st,
                           grad_out, dirn, sdn, idx, slot, V, n, S, C, grad_feat);
    }
    return ured::launch_status("ured_gcn_conv_bwd");
}

int ured_gcn_pool_fwd(const float* feat, const int* idx, const int* sample, int B, int V, int k, int P, int C, float* out,
                      unsigned char* slot, void* stream) {
    ured::clear_error();
    if (const int rc = pool_check("ured_gcn_pool_fwd", B, V, k, P, C)) return rc;
    if (B == 0 || P == 0) return 0;
    URED_REQUIRE(feat && idx && sample && out && slot, "ured_gcn_pool_fwd: null pointer");
    const long long total = (long long)B * P * C;
    hipLaunchKernelGGL(gcn_pool_fwd_kernel, dim3((unsigned)((total + GC_T - 1) / GC_T)), dim3(GC_T), 0, (hipStream_t)stream,
                       feat, idx, sample, V, k, P, C, (u32)total, out, slot);
    return ured::launch_status("ured_gcn_pool_fwd");
}

int ured_gcn_pool_bwd(const float* grad_out, const int* idx, const int* sample, const unsigned char* slot, int B, int V,
                      int k, int P, int C, float* grad_feat, void* stream) {
    ured::clear_error();
    if (const int rc = pool_check("ured_gcn_pool_bwd", B, V, k, P, C)) return rc;
    if (B == 0) return 0;
    URED_REQUIRE(grad_feat && idx && (P == 0 || (grad_out && sample && slot)), "ured_gcn_pool_bwd: null pointer");
    hipLaunchKernelGGL(gcn_pool_bwd_kernel, dim3((V + GC_P - 1) / GC_P, (C + GC_C - 1) / GC_C, B), dim3(64), 0,
                       (hipStream_t)stream, grad_out, idx, sample, slot, V, k, P, C, grad_feat);
    return ured::launch_status("ured_gcn_pool_bwd");
}

}  // extern "C"

URED_DBG_ACCESSOR(ured_dbg_gcn)
