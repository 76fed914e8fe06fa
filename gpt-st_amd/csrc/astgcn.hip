// The downstream ASTGCN predictor (reference model/ASTGCN/ASTGCN.py; gpt-st_amd/predictors/astgcn.py) on HIP: the launches the other
// predictors' kernels cannot make.  Layout as in stgcn.hip: a row is (b, t, n), an activation is (B*T*N rows, C), no permute is materialised.
//
//   attmix     node mixing with a PER-SAMPLE graph M_k[b] = T_k * S_b (Hadamard), formed on the fly in LDS and never written:
//                expand  Out[(b,t,n), k c + ch] = sum_m T_k[m,n] S[b,m,n] In[(b,t,m), ch]                 (the forward: the mask transposed)
//                reduce  Out[(b,t,m), ch]       = sum_k sum_n T_k[m,n] S[b,m,n] In[(b,t,n), k c + ch] + R  (the data backward)
//              A workgroup owns (b, one 16-node output tile) and walks t: its masked tiles (ks x Np x 16) are built once and serve all T steps.
//   attgrad    dS[b,m,n] = sum_k T_k[m,n] sum_{t,ch} X[(b,t,m), ch] G[(b,t,n), k c + ch]: a (N x T c) x (T c x N) product per (b, k), one owner
//              per output element (no reduction over the batch: no partials, no split)
//   rowln      LayerNorm over the c values of one row: 16 lanes per row, 16 rows per 256-thread pass
//
// fp32 MFMA 16x16x4 throughout (exact fp32).  Plain launches only: no workgroup waits on another, nothing is accumulated with float atomics.
#include "common.h"
#include "gptst_hip.h"

#define AG_MP 20            // pitch of a masked tile's rows [q][16 r]: 4 * 20 mod 32 = 16, the two k-rows of a half-wave read disjoint banks
#define AG_SP 68            // pitch of the 64-channel slab: 4 * 68 mod 32 = 16 likewise
#define AG_MAXK 3
#define AG_PRE 20          // float4 per thread of a prefetched slab: Np * 16 / 256, Np <= 320

struct AgMix { const float* Tp; int Np; int ks; const float* S; const float* In; float* Out; const float* R; int c; int reduce; int T; int N; };

// LDS: Ml[ks][Np][AG_MP]  (q = the node summed over, r = the output node within the tile), slab[Np][AG_SP] (64 channels of the (b, t) unit's rows)
// wave w owns the channel tile w of the current 64-channel group; expand keeps one accumulator per k, reduce alternates two over the ks slabs of a group
template <int KS, bool RED>
__global__ __launch_bounds__(256) void ag_attmix_kernel(AgMix p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* Ml = smem;
    float* slab = smem + (size_t)KS * p.Np * AG_MP;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, kk = lane >> 4;
    const int b = blockIdx.y, r0 = blockIdx.x * 16;
    const float* Sb = p.S + (size_t)b * p.N * p.N;
    // ---- the masked tiles of this (b, node tile), once ----
    if (!RED) {                                        // Ml[k][q = m][r] = T_k[m][r0 + r] S[b][m][r0 + r]
#pragma unroll 4
        for (int f = tid; f < KS * p.Np * 16; f += 256) {
            const int r = f & 15, q = (f >> 4) % p.Np, k = (f >> 4) / p.Np, n = r0 + r;
            const float v = (q < p.N && n < p.N) ? p.Tp[((size_t)k * p.Np + q) * p.Np + n] * Sb[(size_t)q * p.N + n] : 0.f;
            Ml[((size_t)k * p.Np + q) * AG_MP + r] = v;
        }
    } else {                                           // Ml[k][q = n][r] = T_k[r0 + r][n] S[b][r0 + r][n]
#pragma unroll 4
        for (int f = tid; f < KS * 16 * p.Np; f += 256) {
            const int q = f % p.Np, r = (f / p.Np) & 15, k = f / (16 * p.Np), m = r0 + r;
            const float v = (q < p.N && m < p.N) ? p.Tp[((size_t)k * p.Np + m) * p.Np + q] * Sb[(size_t)m * p.N + q] : 0.f;
            Ml[((size_t)k * p.Np + q) * AG_MP + r] = v;
        }
    }
    const int ldi = RED ? KS * p.c : p.c, ldo = RED ? p.c : KS * p.c;
    constexpr int nslab = RED ? KS : 1;
    const int ncg = (p.c + 63) / 64, total = p.T * ncg * nslab;
    // the slabs are walked as one sequence it = (t, channel group, slab of the group); the next slab's global loads are in flight (registers)
    // while this one is multiplied: with one workgroup per CU nothing else would hide them
    float4 pre[AG_PRE];
    auto fetch = [&](int it) {
        const int s = it % nslab, cg = (it / nslab) % ncg, t = it / (nslab * ncg);
        const float* src = p.In + ((size_t)b * p.T + t) * p.N * ldi + (RED ? s * p.c : 0) + 64 * cg;
#pragma unroll
        for (int i = 0; i < AG_PRE; ++i) {
            const int f = tid + 256 * i, m = f >> 4, c4 = f & 15;
            pre[i] = (m < p.N && 64 * cg + 4 * c4 < p.c) ? ld4(src + (size_t)m * ldi + 4 * c4) : f4zero();
        }
    };
    f32x4 acc[AG_MAXK];
    fetch(0);
    for (int it = 0; it < total; ++it) {
        const int s = it % nslab, cg = (it / nslab) % ncg, t = it / (nslab * ncg);
        const size_t rbase = ((size_t)b * p.T + t) * p.N;
        __syncthreads();                                        // the previous slab's reads (and, first time, the mask's writes) are done
#pragma unroll
        for (int i = 0; i < AG_PRE; ++i) {
            const int f = tid + 256 * i;
            if (f < p.Np * 16) st4(slab + (f >> 4) * AG_SP + 4 * (f & 15), pre[i]);
        }
        __syncthreads();
        if (it + 1 < total) fetch(it + 1);
        if (64 * cg + 16 * wave >= p.c) continue;               // (c is a multiple of 16: a wave's channel tile is all in or all out)
        const int ch = 64 * cg + 16 * wave + j;                 // this lane's output channel
        if (s == 0) {
#pragma unroll
            for (int k = 0; k < AG_MAXK; ++k) acc[k] = (f32x4){0.f, 0.f, 0.f, 0.f};
        }
        const float* sp = slab + (4 * kk) * AG_SP + 16 * wave + j;
        if (!RED) {
            const float* mp = Ml + (4 * kk) * AG_MP + j;
            for (int q0 = 0; q0 < p.Np; q0 += 16) {             // the 4 + 4 KS LDS reads of a step first, then its 4 KS MFMAs
                float bv[4], av[KS][4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    bv[e] = sp[(q0 + e) * AG_SP];
#pragma unroll
                    for (int k = 0; k < KS; ++k) av[k][e] = mp[(k * p.Np + q0 + e) * AG_MP];
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) {
#pragma unroll
                    for (int k = 0; k < KS; ++k) acc[k] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[k][e], bv[e], acc[k], 0, 0, 0);
                }
            }
            // ---- epilogue in the accumulator layout: reg r = (output node r0 + kk*4 + r, channel ch) ----
#pragma unroll
            for (int k = 0; k < KS; ++k) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int n = r0 + kk * 4 + r;
                    if (n < p.N) p.Out[(rbase + n) * ldo + k * p.c + ch] = acc[k][r];
                }
            }
        } else {                                                // two accumulators in turn: the dependent-issue latency of one chain is hidden
            const float* mp = Ml + (s * p.Np + 4 * kk) * AG_MP + j;
#pragma unroll 2
            for (int q0 = 0; q0 < p.Np; q0 += 16) {
                float bv[4], av[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) { bv[e] = sp[(q0 + e) * AG_SP]; av[e] = mp[(q0 + e) * AG_MP]; }
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[e & 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[e], bv[e], acc[e & 1], 0, 0, 0);
            }
            if (s + 1 < nslab) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int n = r0 + kk * 4 + r;
                if (n < p.N) p.Out[(rbase + n) * ldo + ch] = (acc[0][r] + acc[1][r]) + (p.R != nullptr ? p.R[(rbase + n) * p.c + ch] : 0.f);
            }
        }
    }
}

// ---- gradient of the mix with respect to the per-sample graph ----
struct AgGrad { const float* Tp; int Np; int ks; const float* X; const float* G; float* dS; int c; int T; int N; };

// a wave owns the 16 x 16 tile (m0, n0) of sample b and one accumulator per k; both operands come from global memory in the MFMA's own
// lane layout (lane (j, kk) loads the float4 at channels 16 q + 4 kk of row j): X as A, G as B.  L2 serves the reuse between waves.
template <int KS>
__global__ __launch_bounds__(256) void ag_attgrad_kernel(AgGrad p) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, kk = lane >> 4;
    const int b = blockIdx.z, m0 = blockIdx.y * 16, n0 = (blockIdx.x * 4 + wave) * 16;
    if (n0 >= p.Np) return;                                     // (no barrier in this kernel)
    const int m = m0 + j, n = n0 + j, ldg = KS * p.c;
    const bool mv = m < p.N, nv = n < p.N;
    f32x4 acc[AG_MAXK];
#pragma unroll
    for (int k = 0; k < AG_MAXK; ++k) acc[k] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int t = 0; t < p.T; ++t) {
        const size_t rbase = ((size_t)b * p.T + t) * p.N;
        const float* xp = p.X + (rbase + m) * p.c + 4 * kk;
        const float* gp = p.G + (rbase + n) * ldg + 4 * kk;
        for (int q = 0; q < p.c; q += 16) {
            const float4 a = mv ? ld4(xp + q) : f4zero();
            float4 gk[KS];
#pragma unroll
            for (int k = 0; k < KS; ++k) gk[k] = nv ? ld4(gp + k * p.c + q) : f4zero();
#pragma unroll
            for (int k = 0; k < KS; ++k) {
                const float4 g = gk[k];
                acc[k] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, g.x, acc[k], 0, 0, 0);
                acc[k] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, g.y, acc[k], 0, 0, 0);
                acc[k] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, g.z, acc[k], 0, 0, 0);
                acc[k] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, g.w, acc[k], 0, 0, 0);
            }
        }
    }
    // reg r = (m0 + kk*4 + r, n0 + j)
    if (!nv) return;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int mo = m0 + kk * 4 + r;
        if (mo >= p.N) continue;
        float v = 0.f;
#pragma unroll
        for (int k = 0; k < KS; ++k) v = fmaf(p.Tp[((size_t)k * p.Np + mo) * p.Np + n], acc[k][r], v);
        p.dS[((size_t)b * p.N + mo) * p.N + n] = v;
    }
}

// ---- LayerNorm over the c <= 128 values of a row: 16 lanes per row, two float4 per lane at most ----
__global__ __launch_bounds__(256) void ag_rowln_fwd_kernel(const float* __restrict__ X, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                           float* __restrict__ Y, float* __restrict__ mean, float* __restrict__ rstd, long rows,
                                                           int c, float eps) {
    const int l = threadIdx.x & 15, c0 = 4 * l, c1 = 64 + 4 * l;
    const bool h0 = c0 < c, h1 = c1 < c;
    const float4 g0 = h0 ? ld4(gamma + c0) : f4zero(), g1 = h1 ? ld4(gamma + c1) : f4zero();
    const float4 b0 = h0 ? ld4(beta + c0) : f4zero(), b1 = h1 ? ld4(beta + c1) : f4zero();
    for (long row = (long)blockIdx.x * 16 + (threadIdx.x >> 4); row < rows; row += (long)gridDim.x * 16) {
        const float* x = X + row * c;
        const float4 v0 = h0 ? ld4(x + c0) : f4zero(), v1 = h1 ? ld4(x + c1) : f4zero();
        const float mu = group_sum<16>(((v0.x + v0.y) + (v0.z + v0.w)) + ((v1.x + v1.y) + (v1.z + v1.w))) / (float)c;
        float q = 0.f;
        if (h0) { const float a = v0.x - mu, b = v0.y - mu, d = v0.z - mu, e = v0.w - mu; q += (a * a + b * b) + (d * d + e * e); }
        if (h1) { const float a = v1.x - mu, b = v1.y - mu, d = v1.z - mu, e = v1.w - mu; q += (a * a + b * b) + (d * d + e * e); }
        const float rs = 1.f / sqrtf(group_sum<16>(q) / (float)c + eps);
        if (l == 0 && mean != nullptr) { mean[row] = mu; rstd[row] = rs; }
        float* y = Y + row * c;
        if (h0) st4(y + c0, make_float4(fmaf((v0.x - mu) * rs, g0.x, b0.x), fmaf((v0.y - mu) * rs, g0.y, b0.y), fmaf((v0.z - mu) * rs, g0.z, b0.z), fmaf((v0.w - mu) * rs, g0.w, b0.w)));
        if (h1) st4(y + c1, make_float4(fmaf((v1.x - mu) * rs, g1.x, b1.x), fmaf((v1.y - mu) * rs, g1.y, b1.y), fmaf((v1.z - mu) * rs, g1.z, b1.z), fmaf((v1.w - mu) * rs, g1.w, b1.w)));
    }
}

// dX = rstd (g - mean(g) - xhat mean(g xhat)),  g = dY gamma,  xhat = (x - mean) rstd
__global__ __launch_bounds__(256) void ag_rowln_bwd_kernel(const float* __restrict__ dY, const float* __restrict__ X, const float* __restrict__ gamma,
                                                           const float* __restrict__ mean, const float* __restrict__ rstd, float* __restrict__ dX,
                                                           long rows, int c) {
    const int l = threadIdx.x & 15;
    const int cs[2] = {4 * l, 64 + 4 * l};
    float4 gm[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) gm[h] = cs[h] < c ? ld4(gamma + cs[h]) : f4zero();
    for (long row = (long)blockIdx.x * 16 + (threadIdx.x >> 4); row < rows; row += (long)gridDim.x * 16) {
        const float mu = mean[row], rs = rstd[row];
        float4 g[2], xh[2];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const bool v = cs[h] < c;
            const float4 d = v ? ld4(dY + row * c + cs[h]) : f4zero(), x = v ? ld4(X + row * c + cs[h]) : f4zero();
            g[h] = make_float4(d.x * gm[h].x, d.y * gm[h].y, d.z * gm[h].z, d.w * gm[h].w);
            xh[h] = v ? make_float4((x.x - mu) * rs, (x.y - mu) * rs, (x.z - mu) * rs, (x.w - mu) * rs) : f4zero();
            s1 += (g[h].x + g[h].y) + (g[h].z + g[h].w);
            s2 += (g[h].x * xh[h].x + g[h].y * xh[h].y) + (g[h].z * xh[h].z + g[h].w * xh[h].w);
        }
        const float m1 = group_sum<16>(s1) / (float)c, m2 = group_sum<16>(s2) / (float)c;
#pragma unroll
        for (int h = 0; h < 2; ++h)
            if (cs[h] < c)
                st4(dX + row * c + cs[h], make_float4(rs * (g[h].x - m1 - xh[h].x * m2), rs * (g[h].y - m1 - xh[h].y * m2),
                                                      rs * (g[h].z - m1 - xh[h].z * m2), rs * (g[h].w - m1 - xh[h].w * m2)));
    }
}

// pg[z][e] = sum over the rows of split z of dY xhat,  pb[z][e] = sum of dY: thread (rl, e) walks the rows rl, rl + 256 / c, ... of the split in
// ascending order, then the 256 / c lanes of a column are added in ascending order
__global__ __launch_bounds__(256) void ag_rowln_bwd_param_kernel(const float* __restrict__ dY, const float* __restrict__ X, const float* __restrict__ mean,
                                                                 const float* __restrict__ rstd, float* __restrict__ pg, float* __restrict__ pb,
                                                                 long rows, int c, long rps) {
    __shared__ float sg[256], sb[256];
    const int tid = threadIdx.x, nrl = 256 / c, rl = tid / c, e = tid - rl * c, z = blockIdx.x;
    const long r0 = (long)z * rps, r1 = min(rows, r0 + rps);
    float ag = 0.f, ab = 0.f;
    if (rl < nrl) {
        for (long row = r0 + rl; row < r1; row += nrl) {
            const float d = dY[row * c + e];
            ag = fmaf(d, (X[row * c + e] - mean[row]) * rstd[row], ag);
            ab += d;
        }
    }
    sg[tid] = ag; sb[tid] = ab;
    __syncthreads();
    if (tid < c) {
        float tg = 0.f, tb = 0.f;
        for (int i = 0; i < nrl; ++i) { tg += sg[i * c + tid]; tb += sb[i * c + tid]; }
        pg[(size_t)z * c + tid] = tg;
        pb[(size_t)z * c + tid] = tb;
    }
}

// ---- entry points ----
static size_t ag_mix_smem(int Np, int ks) { return ((size_t)ks * Np * AG_MP + (size_t)Np * AG_SP) * sizeof(float); }
// the (Np, ks) the mix serves: the prefetch array holds a slab of Np <= 16 AG_PRE rows, the masked tiles and the slab fit the 160 KB of a CU
static bool ag_mix_fits(int Np, int ks) { return Np <= 16 * AG_PRE && ks <= AG_MAXK && ag_mix_smem(Np, ks) <= 160 * 1024; }

// (include/gptst_hip_testing.h) bytes of dynamic LDS of the launch gptst_astgcn_attmix makes for this shape
extern "C" int gptst_astgcn_attmix_lds(int Np, int ks) {
    if (Np <= 0 || ks <= 0) return GPTST_EARG;
    if (Np % 16 || !ag_mix_fits(Np, ks)) return GPTST_ESHAPE;
    return (int)ag_mix_smem(Np, ks);
}

extern "C" int gptst_astgcn_attmix(const float* Tp, int Np, int ks, const float* S, const float* In, float* Out, const float* R, int c, int reduce,
                                   int B, int T, int N, void* stream) {
    if (!Tp || !S || !In || !Out || B <= 0 || T <= 0 || N <= 0 || ks <= 0 || (R != nullptr && !reduce)) return GPTST_EARG;
    if (Np != 16 * ((N + 15) / 16) || !ag_mix_fits(Np, ks) || c < 16 || c % 16 || B > 65535) return GPTST_ESHAPE;
    const size_t smem = ag_mix_smem(Np, ks);
    typedef void (*kern_t)(AgMix);
    static const kern_t kerns[2][AG_MAXK] = {{ag_attmix_kernel<1, false>, ag_attmix_kernel<2, false>, ag_attmix_kernel<3, false>},
                                             {ag_attmix_kernel<1, true>, ag_attmix_kernel<2, true>, ag_attmix_kernel<3, true>}};
    const kern_t kern = kerns[reduce ? 1 : 0][ks - 1];
    if (smem > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
        if (e != hipSuccess) return (int)e;
    }
    AgMix p{Tp, Np, ks, S, In, Out, R, c, reduce, T, N};
    hipLaunchKernelGGL(kern, dim3(Np / 16, B), dim3(256), smem, (hipStream_t)stream, p);
    GPTST_CHECK_LAUNCH();
    return GPTST_OK;
}

extern "C" int gptst_astgcn_attgrad(const float* Tp, int Np, int ks, const float* X, const float* G, float* dS, int c, int B, int T, int N,
                                    void* stream) {
    if (!Tp || !X || !G || !dS || B <= 0 || T <= 0 || N <= 0 || ks <= 0) return GPTST_EARG;
    if (Np != 16 * ((N + 15) / 16) || ks > AG_MAXK || c < 16 || c % 16 || B > 65535 || Np / 16 > 65535) return GPTST_ESHAPE;
    AgGrad p{Tp, Np, ks, X, G, dS, c, T, N};
    const dim3 grid((Np / 16 + 3) / 4, Np / 16, B);
    if (ks == 1) hipLaunchKernelGGL(ag_attgrad_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, p);
    else if (ks == 2) hipLaunchKernelGGL(ag_attgrad_kernel<2>, grid, dim3(256), 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(ag_attgrad_kernel<3>, grid, dim3(256), 0, (hipStream_t)stream, p);
    GPTST_CHECK_LAUNCH();
    return GPTST_OK;
}

static unsigned ag_rowln_blocks(long rows) {
    long blocks = (rows + 15) / 16;
    return (unsigned)(blocks > 8192 ? 8192 : blocks);
}

extern "C" int gptst_astgcn_rowln_fwd(const float* X, const float* gamma, const float* beta, float* Y, float* mean, float* rstd, long rows, int c,
                                      float eps, void* stream) {
    if (!X || !gamma || !beta || !Y || rows <= 0 || (mean != nullptr) != (rstd != nullptr)) return GPTST_EARG;
    if (c < 16 || c % 16 || c > 128) return GPTST_ESHAPE;
    hipLaunchKernelGGL(ag_rowln_fwd_kernel, dim3(ag_rowln_blocks(rows)), dim3(256), 0, (hipStream_t)stream, X, gamma, beta, Y, mean, rstd, rows, c, eps);
    GPTST_CHECK_LAUNCH();
    return GPTST_OK;
}

extern "C" int gptst_astgcn_rowln_bwd(const float* dY, const float* X, const float* gamma, const float* mean, const float* rstd, float* dX, long rows,
                                      int c, void* stream) {
    if (!dY || !X || !gamma || !mean || !rstd || !dX || rows <= 0) return GPTST_EARG;
    if (c < 16 || c % 16 || c > 128) return GPTST_ESHAPE;
    hipLaunchKernelGGL(ag_rowln_bwd_kernel, dim3(ag_rowln_blocks(rows)), dim3(256), 0, (hipStream_t)stream, dY, X, gamma, mean, rstd, dX, rows, c);
    GPTST_CHECK_LAUNCH();
    return GPTST_OK;
}

extern "C" int gptst_astgcn_rowln_nsplit(long rows) {
    if (rows <= 0) return GPTST_EARG;
    const long want = (rows + 255) / 256;                        // at least 256 rows per split
    const long ns = want > 256 ? 256 : want, rps = (rows + ns - 1) / ns;
    return (int)((rows + rps - 1) / rps);
}

extern "C" int gptst_astgcn_rowln_bwd_param(const float* dY, const float* X, const float* mean, const float* rstd, float* pg, float* pb, int nsplit,
                                            long rows, int c, void* stream) {
    if (!dY || !X || !mean || !rstd || !pg || !pb || rows <= 0 || nsplit != gptst_astgcn_rowln_nsplit(rows)) return GPTST_EARG;
    if (c < 16 || c % 16 || c > 128) return GPTST_ESHAPE;
    const long rps = (rows + nsplit - 1) / nsplit;
    hipLaunchKernelGGL(ag_rowln_bwd_param_kernel, dim3(nsplit), dim3(256), 0, (hipStream_t)stream, dY, X, mean, rstd, pg, pb, rows, c, rps);
    GPTST_CHECK_LAUNCH();
    return GPTST_OK;
}
