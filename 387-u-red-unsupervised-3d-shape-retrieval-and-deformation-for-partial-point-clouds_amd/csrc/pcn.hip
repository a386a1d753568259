// pcn.hip — the kernels of the PCN completion network that are not GEMMs, for MI355X / gfx950
// (Density_aware_Chamfer_Distance/models/pcn.py:13-71). Activations are point-major [rows][C] fp32.
//
//   ured_pcn_relu      out = max(y, 0), or with a gradient g: out = y > 0 ? g : 0 (the ReLU backward
//                      of the bias-only layers).
//   ured_pcn_pool_bwd  the backward of a max over the rows of each group: the winner alone takes
//                      the gradient. Written (every element of dY set) or added (the winners only).
//   ured_pcn_fold_fwd  the decoder's conv1 pre-activation without its [B, 1029, num_fine] operand:
//                      Y[(b, c, s)] = (Gb[b] + Pc[b, c]) + Gs[s].
//   ured_pcn_fold_bwd  G = dH where Y > 0 else 0, reduced in a fixed order with no float atomics:
//                      over s into dPc[b, c]; over the coarse points of a chunk into ws[chunk][s]
//                      (the caller sums the chunks, and dPc over c into dGb, with the column-sum
//                      kernels of the GEMM library).
//   ured_pcn_center_fwd / _bwd   fine = conv3 output + its coarse point; the sum over s back.
#define URED_DBG_FILE 17
#include "ured_common.h"
#include "../../include/ured_hip.h"

namespace {

constexpr int PCN_THREADS = 256;
constexpr int PCN_MAX_SCALE = 16;     // fine points per coarse point (accumulators in registers)

__global__ __launch_bounds__(PCN_THREADS) void pcn_relu_kernel(const float* __restrict__ y, const float* __restrict__ g,
                                                               long long n, int vec, float* __restrict__ out) {
    const long long i = ((long long)blockIdx.x * PCN_THREADS + threadIdx.x) * 4;
    if (i >= n) return;
    if (vec && i + 4 <= n) {
        const float4 v = *reinterpret_cast<const float4*>(y + i);
        float4 o;
        if (g) {
            const float4 u = *reinterpret_cast<const float4*>(g + i);
            o.x = v.x > 0.f ? u.x : 0.f; o.y = v.y > 0.f ? u.y : 0.f;
            o.z = v.z > 0.f ? u.z : 0.f; o.w = v.w > 0.f ? u.w : 0.f;
        } else {
            o.x = fmaxf(v.x, 0.f); o.y = fmaxf(v.y, 0.f); o.z = fmaxf(v.z, 0.f); o.w = fmaxf(v.w, 0.f);
        }
        *reinterpret_cast<float4*>(out + i) = o;
        return;
    }
    for (long long k = i; k < n && k < i + 4; ++k) out[k] = g ? (y[k] > 0.f ? g[k] : 0.f) : fmaxf(y[k], 0.f);
}

// written form: one thread per element of dY
__global__ __launch_bounds__(PCN_THREADS) void pcn_pool_bwd_set_kernel(const float* __restrict__ g, const int* __restrict__ win,
                                                                       int rows, int C, long long total,
                                                                       float* __restrict__ dY) {
    const long long i = (long long)blockIdx.x * PCN_THREADS + threadIdx.x;
    if (i >= total) return;
    const long long r = i / C;
    const int c = (int)(i - r * C);
    const long long grp = r / rows;
    const int w = win[grp * C + c];
    URED_DBG_CHECK((long long)w >= grp * rows && (long long)w < (grp + 1) * rows);
    dY[i] = (long long)w == r ? g[grp * C + c] : 0.f;
}

// added form: one thread per (group, channel); distinct threads own distinct elements
__global__ __launch_bounds__(PCN_THREADS) void pcn_pool_bwd_add_kernel(const float* __restrict__ g, const int* __restrict__ win,
                                                                       int G, int rows, int C, float* __restrict__ dY) {
    const long long i = (long long)blockIdx.x * PCN_THREADS + threadIdx.x;
    if (i >= (long long)G * C) return;
    const long long grp = i / C;
    const int c = (int)(i - grp * C);
    const long long w = win[i];
    const bool ok = w >= grp * rows && w < (grp + 1) * rows;
    URED_DBG_CHECK(ok);
    if (ok) dY[w * C + c] += g[i];       // a winner outside its group is never written
}

__global__ __launch_bounds__(PCN_THREADS) void pcn_fold_fwd_kernel(const float* __restrict__ Gb, const float* __restrict__ Pc,
                                                                   const float* __restrict__ Gs, int nc, int S, int C,
                                                                   long long total, float* __restrict__ Y) {
    const long long i = (long long)blockIdx.x * PCN_THREADS + threadIdx.x;
    if (i >= total) return;
    const long long r = i / C;
    const int c = (int)(i - r * C);
    const long long bc = r / S;
    const int s = (int)(r - bc * S);
    const long long b = bc / nc;
    Y[i] = (Gb[b * C + c] + Pc[bc * C + c]) + Gs[(long long)s * C + c];
}

// One workgroup per chunk of consecutive coarse points (b, c flattened); a thread owns channels
// t, t + 256, ... and walks the chunk's points and their S fine points in ascending order.
__global__ __launch_bounds__(PCN_THREADS) void pcn_fold_bwd_kernel(const float* __restrict__ dH, const float* __restrict__ Y,
                                                                   long long npts, int S, int C, int chunk,
                                                                   float* __restrict__ dPc, float* __restrict__ ws) {
    const long long p0 = (long long)blockIdx.x * chunk;
    const long long p1 = p0 + chunk < npts ? p0 + chunk : npts;
    for (int c = threadIdx.x; c < C; c += PCN_THREADS) {
        float gs[PCN_MAX_SCALE];
#pragma unroll
        for (int s = 0; s < PCN_MAX_SCALE; ++s) gs[s] = 0.f;
        for (long long p = p0; p < p1; ++p) {
            float acc = 0.f;
#pragma unroll
            for (int s = 0; s < PCN_MAX_SCALE; ++s) {
                if (s < S) {
                    const long long e = (p * S + s) * C + c;
                    const float g = Y[e] > 0.f ? dH[e] : 0.f;
                    acc += g;
                    gs[s] += g;
                }
            }
            dPc[p * C + c] = acc;
        }
#pragma unroll
        for (int s = 0; s < PCN_MAX_SCALE; ++s)
            if (s < S) ws[((long long)blockIdx.x * S + s) * C + c] = gs[s];
    }
}

__global__ __launch_bounds__(PCN_THREADS) void pcn_center_fwd_kernel(const float* __restrict__ y, const float* __restrict__ cp,
                                                                     long long total, int S, float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * PCN_THREADS + threadIdx.x;
    if (i >= total) return;
    const long long r = i / 3;
    const int k = (int)(i - r * 3);
    out[i] = y[i] + cp[(r / S) * 3 + k];
}

__global__ __launch_bounds__(PCN_THREADS) void pcn_center_bwd_kernel(const float* __restrict__ dF, const float* __restrict__ add,
                                                                     long long total, int S, float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * PCN_THREADS + threadIdx.x;
    if (i >= total) return;
    const long long q = i / 3;
    const int k = (int)(i - q * 3);
    float acc = 0.f;
    for (int s = 0; s < S; ++s) acc += dF[(q * S + s) * 3 + k];
    out[i] = add ? acc + add[i] : acc;
}

inline unsigned blocks_for(long long n) { return (unsigned)((n + PCN_THREADS - 1) / PCN_THREADS); }
constexpr long long PCN_MAX_ELEMS = (1LL << 31) * PCN_THREADS / 2;   // grid.x stays below 2^30 blocks

}  // namespace

extern "C" {

int ured_pcn_relu(const float* y, const float* g, long long n, float* out, void* stream) {
    ured::clear_error();
    URED_REQUIRE(n >= 0 && n < PCN_MAX_ELEMS, "ured_pcn_relu: bad size %lld", n);
    if (n == 0) return 0;
    URED_REQUIRE(y && out, "ured_pcn_relu: null pointer");
    const int vec = (((uintptr_t)y | (uintptr_t)g | (uintptr_t)out) & 15) == 0;
    hipLaunchKernelGGL(pcn_relu_kernel, dim3(blocks_for((n + 3) / 4)), dim3(PCN_THREADS), 0, (hipStream_t)stream, y, g, n,
                       vec, out);
    return ured::launch_status("ured_pcn_relu");
}

int ured_pcn_pool_bwd(const float* g, const int* win, int G, int rows, int C, float* dY, int accumulate, void* stream) {
    ured::clear_error();
    URED_REQUIRE(G >= 0 && rows > 0 && C > 0, "ured_pcn_pool_bwd: bad sizes G=%d rows=%d C=%d", G, rows, C);
    const long long total = (long long)G * rows * C;
    URED_REQUIRE(total < PCN_MAX_ELEMS && (long long)G * rows < (1LL << 31), "ured_pcn_pool_bwd: too large");
    if (G == 0) return 0;
    URED_REQUIRE(g && win && dY, "ured_pcn_pool_bwd: null pointer");
    if (accumulate)
        hipLaunchKernelGGL(pcn_pool_bwd_add_kernel, dim3(blocks_for((long long)G * C)), dim3(PCN_THREADS), 0,
                           (hipStream_t)stream, g, win, G, rows, C, dY);
    else
        hipLaunchKernelGGL(pcn_pool_bwd_set_kernel, dim3(blocks_for(total)), dim3(PCN_THREADS), 0, (hipStream_t)stream, g,
                           win, rows, C, total, dY);
    return ured::launch_status("ured_pcn_pool_bwd");
}

int ured_pcn_fold_fwd(const float* Gb, const float* Pc, const float* Gs, int B, int num_coarse, int scale, int C, float* Y,
                      void* stream) {
    ured::clear_error();
    URED_REQUIRE(B >= 0 && num_coarse > 0 && scale > 0 && C > 0, "ured_pcn_fold_fwd: bad sizes B=%d num_coarse=%d scale=%d C=%d",
                 B, num_coarse, scale, C);
    const long long total = (long long)B * num_coarse * scale * C;
    URED_REQUIRE(total < PCN_MAX_ELEMS, "ured_pcn_fold_fwd: too large");
    if (B == 0) return 0;
    URED_REQUIRE(Gb && Pc && Gs && Y, "ured_pcn_fold_fwd: null pointer");
    hipLaunchKernelGGL(pcn_fold_fwd_kernel, dim3(blocks_for(total)), dim3(PCN_THREADS), 0, (hipStream_t)stream, Gb, Pc, Gs,
                       num_coarse, scale, C, total, Y);
    return ured::launch_status("ured_pcn_fold_fwd");
}

int ured_pcn_fold_bwd(const float* dH, const float* Y, int B, int num_coarse, int scale, int C, int chunk, float* dPc,
                      float* ws, void* stream) {
    ured::clear_error();
    URED_REQUIRE(B >= 0 && num_coarse > 0 && C > 0 && chunk > 0, "ured_pcn_fold_bwd: bad sizes B=%d num_coarse=%d C=%d chunk=%d",
                 B, num_coarse, C, chunk);
    URED_REQUIRE(scale > 0 && scale <= PCN_MAX_SCALE, "ured_pcn_fold_bwd: scale %d outside [1, %d]", scale, PCN_MAX_SCALE);
    const long long npts = (long long)B * num_coarse;
    URED_REQUIRE(npts * scale * C < PCN_MAX_ELEMS, "ured_pcn_fold_bwd: too large");
    if (B == 0) return 0;
    URED_REQUIRE(dH && Y && dPc && ws, "ured_pcn_fold_bwd: null pointer");
    hipLaunchKernelGGL(pcn_fold_bwd_kernel, dim3((unsigned)((npts + chunk - 1) / chunk)), dim3(PCN_THREADS), 0,
                       (hipStream_t)stream, dH, Y, npts, scale, C, chunk, dPc, ws);
    return ured::launch_status("ured_pcn_fold_bwd");
}

int ured_pcn_center_fwd(const float* y, const float* cp, int B, int num_coarse, int scale, float* out, void* stream) {
    ured::clear_error();
    URED_REQUIRE(B >= 0 && num_coarse > 0 && scale > 0, "ured_pcn_center_fwd: bad sizes B=%d num_coarse=%d scale=%d", B,
                 num_coarse, scale);
    const long long total = (long long)B * num_coarse * scale * 3;
    URED_REQUIRE(total < PCN_MAX_ELEMS, "ured_pcn_center_fwd: too large");
    if (B == 0) return 0;
    URED_REQUIRE(y && cp && out, "ured_pcn_center_fwd: null pointer");
    hipLaunchKernelGGL(pcn_center_fwd_kernel, dim3(blocks_for(total)), dim3(PCN_THREADS), 0, (hipStream_t)stream, y, cp,
                       total, scale, out);
    return ured::launch_status("ured_pcn_center_fwd");
}

int ured_pcn_center_bwd(const float* dF, const float* add, int B, int num_coarse, int scale, float* out, void* stream) {
    ured::clear_error();
    URED_REQUIRE(B >= 0 && num_coarse > 0 && scale > 0, "ured_pcn_center_bwd: bad sizes B=%d num_coarse=%d scale=%d", B,
                 num_coarse, scale);
    const long long total = (long long)B * num_coarse * 3;
    URED_REQUIRE(total * scale < PCN_MAX_ELEMS, "ured_pcn_center_bwd: too large");
    if (B == 0) return 0;
    URED_REQUIRE(dF && out, "ured_pcn_center_bwd: null pointer");
    hipLaunchKernelGGL(pcn_center_bwd_kernel, dim3(blocks_for(total)), dim3(PCN_THREADS), 0, (hipStream_t)stream, dF, add,
                       total, scale, out);
    return ured::launch_status("ured_pcn_center_bwd");
}

}  // extern "C"

URED_DBG_ACCESSOR(ured_dbg_pcn)
