// The downstream STGCN predictor (reference model/STGCN/stgcn.py; gpt-st_amd/predictors/stgcn.py) on HIP, forward and backward, in the
// channels-last layout the rest of the project uses: a row is (b, t, n), an activation is (B*T*N rows, C), no permute is materialised.
//
//   tapgemm     Y = act(sum_j X[t + dt_j] W_j + b + res)     temporal convolutions ('same' zero padding in T: a tap is a row offset of
//               dt_j * N rows, a tap outside [0, T) is not loaded), their data backward (the taps mirrored, W transposed by the caller),
//               and the two channel GEMMs of the graph convolution.  GLU / relu / sigmoid in the epilogue; the 1x1 align is one more tap.
//               The staging of the weight rows (with the GLU row interleave) is row_gemm_stage (row_gemm_dev.h), shared with
//               ss_wingemm_kernel (stsgcn.hip), and so is the launch plan; the tile loop and the epilogue are this kernel's own.
//   gate_bwd    dPre from dOut and what the forward kept (GLU: sigma(Q) and P + res, stored by glu_bwd_store as in stsgcn.hip; relu /
//               sigmoid: the output itself)
//   wgrad       dW[o][k] = sum_rows dPre[row][o] X_shift[row][k] (rectangular, shifted) + column sums of dPre: row-split partials, fixed order
//   nodemix     per (b, t): Z_k = L_k X (expand) or  Y = sum_k L_k Z_k + R (reduce); a 32-channel slab of the unit in LDS, L_k read from L2
//               (the product is node_mix_slab, node_mix_dev.h, which ss_mix_kernel of stsgcn.hip runs too)
//   ln_fwd/bwd  LayerNorm over (N, C) per (b, t); variance about the mean; dgamma / dbeta as unit-split partials
//
// fp32 MFMA 16x16x4 throughout (exact fp32).  Plain launches only: no workgroup waits on another, nothing is accumulated with float atomics.
#include "common.h"
#include "gptst_hip.h"
#include "node_mix_dev.h"
#include "row_gemm_dev.h"
#include "tap_wgrad_dev.h"

#define SG_ACT_NONE 0
#define SG_ACT_RELU 1
#define SG_ACT_SIGMOID 2
#define SG_ACT_GLU 3
#define SG_MAX_DEVICES 64

struct SgTap { int n; int dt[4]; };

struct SgTg {
    const float* X; int ldx; int ci; SgTap tap;
    const float* W; int Ktot; const float* bias;
    const float* R; int ldr; int res_w;
    float* Y; int co; float* S; float* A; int act;
    int rows, T, N, tpw;
};

// a wave owns 16-row tiles and NCT column tiles of 16; the workgroup's 16*NCT weight rows (all K) sit in LDS, staged by row_gemm_stage
// (row_gemm_dev.h).  GLU: the first NCT/2 tiles are P channels, the other half the Q channels of the same outputs, so a lane holds P and Q of
// one (row, channel) pair.
template <int NCT>
__global__ __launch_bounds__(ROW_GEMM_THREADS) void sg_tapgemm_kernel(SgTg p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int OCW = 16 * NCT, half = OCW / 2;
    const int P = p.Ktot + 4;
    const float* Wl = smem;                 // [OCW][P]
    const float* bl = Wl + OCW * P;         // [OCW]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, kk = lane >> 4;
    const bool glu = p.act == SG_ACT_GLU;
    const int c0 = row_gemm_stage<NCT>(smem, p.W, p.bias, p.Ktot, p.co, glu);
    const int ntiles = (p.rows + 15) / 16, nq = p.ci >> 4;
    const int t0 = (blockIdx.x * (ROW_GEMM_THREADS / 64) + wave) * p.tpw, t1 = min(ntiles, t0 + p.tpw);
    for (int t = t0; t < t1; ++t) {
        const int row0 = t * 16, ra = row0 + j;
        const bool rv = ra < p.rows;
        const int tt = (ra / p.N) % p.T;
        f32x4 acc[NCT];
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) acc[ct] = (f32x4){0.f, 0.f, 0.f, 0.f};
        for (int tp = 0; tp < p.tap.n; ++tp) {
            const int dt = p.tap.dt[tp], ts = tt + dt;
            const bool ok = rv && ts >= 0 && ts < p.T;          // a tap in the padding contributes nothing and is not loaded
            const float* xp = p.X + ((long)ra + (long)dt * p.N) * p.ldx + 4 * kk;
            const float* wl = Wl + j * P + tp * p.ci + 4 * kk;
            for (int q = 0; q < nq; q += 2) {
                const bool two = q + 1 < nq;
                const float4 a0 = ok ? ld4(xp + 16 * q) : f4zero();
                const float4 a1 = (ok && two) ? ld4(xp + 16 * q + 16) : f4zero();
#pragma unroll
                for (int ct = 0; ct < NCT; ++ct) {
                    const float4 b = ld4(wl + 16 * ct * P + 16 * q);
                    acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.x, b.x, acc[ct], 0, 0, 0);
                    acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.y, b.y, acc[ct], 0, 0, 0);
                    acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.z, b.z, acc[ct], 0, 0, 0);
                    acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.w, b.w, acc[ct], 0, 0, 0);
                }
                if (two) {
#pragma unroll
                    for (int ct = 0; ct < NCT; ++ct) {
                        const float4 b = ld4(wl + 16 * ct * P + 16 * q + 16);
                        acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.x, b.x, acc[ct], 0, 0, 0);
                        acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.y, b.y, acc[ct], 0, 0, 0);
                        acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.z, b.z, acc[ct], 0, 0, 0);
                        acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.w, b.w, acc[ct], 0, 0, 0);
                    }
                }
            }
        }
        // ---- epilogue in the accumulator layout: reg r = (row kk*4 + r, column 16 ct + j) ----
        if (glu) {
#pragma unroll
            for (int ct = 0; ct < NCT / 2; ++ct) {
                const int ch = c0 + 16 * ct + j;
                if (ch >= p.co) continue;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = row0 + kk * 4 + r;
                    if (row >= p.rows) continue;
                    float pv = acc[ct][r] + bl[16 * ct + j];
                    if (ch < p.res_w) pv += p.R[(size_t)row * p.ldr + ch];
                    const float s = sigmoidf_(acc[ct + NCT / 2][r] + bl[half + 16 * ct + j]);
                    p.Y[(size_t)row * p.co + ch] = pv * s;
                    if (p.S != nullptr) { p.S[(size_t)row * p.co + ch] = s; p.A[(size_t)row * p.co + ch] = pv; }
                }
            }
        } else {
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) {
                const int ch = c0 + 16 * ct + j;
                if (ch >= p.co) continue;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = row0 + kk * 4 + r;
                    if (row >= p.rows) continue;
                    float v = acc[ct][r] + bl[16 * ct + j];
                    if (ch < p.res_w) v += p.R[(size_t)row * p.ldr + ch];
                    if (p.act == SG_ACT_RELU) v = fmaxf(v, 0.f);
                    else if (p.act == SG_ACT_SIGMOID) v = sigmoidf_(v);
                    p.Y[(size_t)row * p.co + ch] = v;
                }
            }
        }
    }
}

// dPre (rows, co or 2 co) from dOut (rows, co): relu: dOut [out > 0];  sigmoid: dOut out (1 - out);
// GLU (out = A S, A = P + res, S = sigma(Q)): [dOut S | dOut A S (1 - S)]
__global__ __launch_bounds__(256) void sg_gate_bwd_kernel(const float* __restrict__ dOut, const float* __restrict__ out, const float* __restrict__ S,
                                                          const float* __restrict__ A, float* __restrict__ dPre, int act, long n4, int co4) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        const float4 g = ld4(dOut + 4 * i);
        if (act == SG_ACT_GLU) {
            const long row = i / co4;
            const int c4 = (int)(i - row * co4);
            const float4 s = ld4(S + 4 * i), a = ld4(A + 4 * i);
            glu_bwd_store(dPre + (row * 2 * co4 + c4) * 4, co4, g, s, a);
        } else {
            const float4 o = ld4(out + 4 * i);
            if (act == SG_ACT_RELU) st4(dPre + 4 * i, make_float4(o.x > 0.f ? g.x : 0.f, o.y > 0.f ? g.y : 0.f, o.z > 0.f ? g.z : 0.f, o.w > 0.f ? g.w : 0.f));
            else st4(dPre + 4 * i, make_float4(g.x * o.x * (1.f - o.x), g.y * o.y * (1.f - o.y), g.z * o.z * (1.f - o.z), g.w * o.w * (1.f - o.w)));
        }
    }
}

// ---- weight gradient of a tap GEMM: part[z][o][k] = sum over the rows of split z of D[row][o] X_shift[row][k]; bpart[z][o] = column sums of D ----
struct SgWg {
    const float* D; int cw; const float* X; int ldx; int ci; SgTap tap; int Ktot;
    float* part; float* bpart; int rows, T, N, cps, nchunks;
};

// the source of a row for this thread's columns: the row dt * N rows away, where its time step is inside [0, T)
struct SgWgSrc {
    const SgWg& p; bool kv; int xc, dt;
    __device__ __forceinline__ SgWgSrc(const SgWg& p_, int kcol) : p(p_), kv(kcol < p_.Ktot) {
        const int tp = kv ? kcol / p.ci : 0;
        xc = kcol - tp * p.ci; dt = p.tap.dt[tp];
    }
    __device__ __forceinline__ float4 operator()(int row, bool rv) const {
        const int ts = (row / p.N) % p.T + dt;
        return (rv && kv && ts >= 0 && ts < p.T) ? ld4(p.X + ((long)row + (long)dt * p.N) * p.ldx + xc) : f4zero();
    }
};

__global__ __launch_bounds__(256) void sg_wgrad_kernel(SgWg p) {
    tap_wgrad_body(p.D, p.cw, p.Ktot, p.part, p.bpart, p.rows, p.cps, p.nchunks, SgWgSrc(p, blockIdx.x * 64 + 4 * (threadIdx.x & 15)));
}

// ---- node mixing with the Chebyshev polynomials: one (b, t) unit and four 16-node tiles per workgroup ----
// L (ks, Np, Np) zero-padded to Np = 16 ceil(N / 16);  expand: Out[:, k c + ch] = (L_k In)[:, ch];  reduce: Out = sum_k L_k In[:, k c + ch] + R
struct SgNm { const float* L; int Np; int ks; const float* In; float* Out; const float* R; int c; int reduce; int N; };

__global__ __launch_bounds__(256) void sg_nodemix_kernel(SgNm p) {
    extern __shared__ __attribute__((aligned(16))) float slab[];            // [Np][NODE_MIX_P]: 32 channels of the unit's rows
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, kk = lane >> 4;
    const int unit = blockIdx.x, nt = blockIdx.y * 4 + wave, n0 = nt * 16;
    const bool active = n0 < p.Np;
    const int ldi = p.reduce ? p.ks * p.c : p.c, ldo = p.reduce ? p.c : p.ks * p.c;
    const size_t rbase = (size_t)unit * p.N;
    for (int cg = 0; cg * 32 < p.c; ++cg) {
        f32x4 acc[2];
        acc[0] = acc[1] = (f32x4){0.f, 0.f, 0.f, 0.f};
        for (int k = 0; k < p.ks; ++k) {
            if (p.reduce || k == 0) {
                __syncthreads();
                const int col0 = (p.reduce ? k * p.c : 0) + 32 * cg;
                for (int f = tid; f < p.Np * 8; f += 256) {
                    const int m = f >> 3, c4 = f & 7;
                    const bool v = m < p.N && 32 * cg + 4 * c4 < p.c;
                    st4(slab + m * NODE_MIX_P + 4 * c4, v ? ld4(p.In + (rbase + m) * ldi + col0 + 4 * c4) : f4zero());
                }
                __syncthreads();
            }
            if (!active) continue;
            if (!p.reduce) acc[0] = acc[1] = (f32x4){0.f, 0.f, 0.f, 0.f};
            node_mix_slab(acc, p.L + ((size_t)k * p.Np + n0 + j) * p.Np + 4 * kk, slab, p.Np, j, kk);
            if (!p.reduce) {
#pragma unroll
                for (int ct = 0; ct < 2; ++ct) {
                    const int ch = 32 * cg + 16 * ct + j;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int n = n0 + kk * 4 + r;
                        if (n < p.N && ch < p.c) p.Out[(rbase + n) * ldo + k * p.c + ch] = acc[ct][r];
                    }
                }
            }
        }
        if (p.reduce && active) {
#pragma unroll
            for (int ct = 0; ct < 2; ++ct) {
                const int ch = 32 * cg + 16 * ct + j;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int n = n0 + kk * 4 + r;
                    if (n < p.N && ch < p.c) p.Out[(rbase + n) * ldo + ch] = acc[ct][r] + (p.R != nullptr ? p.R[(rbase + n) * p.c + ch] : 0.f);
                }
            }
        }
    }
}

// ---- LayerNorm over the M = N C values of a (b, t) unit ----
// sums of two values over a 256-thread workgroup, in a fixed order; every thread gets both totals
__device__ __forceinline__ void sg_block_sum2(float& a, float& b, float* red) {
    a = group_sum<64>(a); b = group_sum<64>(b);
    const int wave = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { red[wave] = a; red[4 + wave] = b; }
    __syncthreads();
    a = ((red[0] + red[1]) + red[2]) + red[3];
    b = ((red[4] + red[5]) + red[6]) + red[7];
}

__global__ __launch_bounds__(256) void sg_ln_fwd_kernel(const float* __restrict__ X, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                        float* __restrict__ Y, float* __restrict__ mean, float* __restrict__ rstd, int M, float eps) {
    __shared__ float red[8];
    const int u = blockIdx.x, tid = threadIdx.x, m4 = M >> 2;
    const float* x = X + (size_t)u * M;
    float s = 0.f, z = 0.f;
    for (int i = tid; i < m4; i += 256) { const float4 v = ld4(x + 4 * i); s += (v.x + v.y) + (v.z + v.w); }
    sg_block_sum2(s, z, red);
    const float mu = s / (float)M;
    float q = 0.f;
    for (int i = tid; i < m4; i += 256) {
        const float4 v = ld4(x + 4 * i);
        const float a = v.x - mu, b = v.y - mu, c = v.z - mu, d = v.w - mu;
        q += (a * a + b * b) + (c * c + d * d);
    }
    z = 0.f;
    sg_block_sum2(q, z, red);
    const float rs = 1.f / sqrtf(q / (float)M + eps);
    if (tid == 0 && mean != nullptr) { mean[u] = mu; rstd[u] = rs; }
    float* y = Y + (size_t)u * M;
    for (int i = tid; i < m4; i += 256) {
        const float4 v = ld4(x + 4 * i), g = ld4(gamma + 4 * i), b = ld4(beta + 4 * i);
        st4(y + 4 * i, make_float4(fmaf((v.x - mu) * rs, g.x, b.x), fmaf((v.y - mu) * rs, g.y, b.y), fmaf((v.z - mu) * rs, g.z, b.z), fmaf((v.w - mu) * rs, g.w, b.w)));
    }
}

// dX = rstd (g - mean(g) - xhat mean(g xhat)),  g = dY gamma,  xhat = (x - mean) rstd
__global__ __launch_bounds__(256) void sg_ln_bwd_kernel(const float* __restrict__ dY, const float* __restrict__ X, const float* __restrict__ gamma,
                                                        const float* __restrict__ mean, const float* __restrict__ rstd, float* __restrict__ dX, int M) {
    __shared__ float red[8];
    const int u = blockIdx.x, tid = threadIdx.x, m4 = M >> 2;
    const float* x = X + (size_t)u * M;
    const float* dy = dY + (size_t)u * M;
    const float mu = mean[u], rs = rstd[u];
    float s1 = 0.f, s2 = 0.f;
    for (int i = tid; i < m4; i += 256) {
        const float4 v = ld4(x + 4 * i), d = ld4(dy + 4 * i), g = ld4(gamma + 4 * i);
        const float g0 = d.x * g.x, g1 = d.y * g.y, g2 = d.z * g.z, g3 = d.w * g.w;
        s1 += (g0 + g1) + (g2 + g3);
        s2 += (g0 * ((v.x - mu) * rs) + g1 * ((v.y - mu) * rs)) + (g2 * ((v.z - mu) * rs) + g3 * ((v.w - mu) * rs));
    }
    sg_block_sum2(s1, s2, red);
    const float m1 = s1 / (float)M, m2 = s2 / (float)M;
    float* dx = dX + (size_t)u * M;
    for (int i = tid; i < m4; i += 256) {
        const float4 v = ld4(x + 4 * i), d = ld4(dy + 4 * i), g = ld4(gamma + 4 * i);
        st4(dx + 4 * i, make_float4(rs * (d.x * g.x - m1 - (v.x - mu) * rs * m2), rs * (d.y * g.y - m1 - (v.y - mu) * rs * m2),
                                    rs * (d.z * g.z - m1 - (v.z - mu) * rs * m2), rs * (d.w * g.w - m1 - (v.w - mu) * rs * m2)));
    }
}

// pg[z][e] = sum over the units of split z of dY xhat,  pb[z][e] = sum of dY   (e < M), units in ascending order
__global__ __launch_bounds__(256) void sg_ln_bwd_param_kernel(const float* __restrict__ dY, const float* __restrict__ X, const float* __restrict__ mean,
                                                              const float* __restrict__ rstd, float* __restrict__ pg, float* __restrict__ pb, int units,
                                                              int M, int ups) {
    const int e = blockIdx.x * 256 + threadIdx.x, z = blockIdx.y;
    if (e >= M) return;
    const int u0 = z * ups, u1 = min(units, u0 + ups);
    float sg = 0.f, sb = 0.f;
#pragma unroll 4
    for (int u = u0; u < u1; ++u) {
        const float d = dY[(size_t)u * M + e];
        sg = fmaf(d, (X[(size_t)u * M + e] - mean[u]) * rstd[u], sg);
        sb += d;
    }
    pg[(size_t)z * M + e] = sg;
    pb[(size_t)z * M + e] = sb;
}

// ---- entry points ----
static bool sg_taps_ok(int ntap, const int* dt, int T) {
    if (ntap < 1 || ntap > 4) return false;
    for (int i = 0; i < ntap; ++i) if (dt[i] <= -T || dt[i] >= T) return false;
    return true;
}

// the launch plan of the tap GEMM: 64 weight rows of up to 388 floats (99 KB), beyond that 32 rows; about 512 workgroups
static RowGemmPlan sg_tapgemm_plan(int rows, int co, int Ktot, int act) {
    return row_gemm_plan((rows + 15) / 16, co, act == SG_ACT_GLU, Ktot <= 384, 1, 512);
}

// (include/gptst_hip_testing.h) tiles per wave of the launch gptst_stgcn_tapgemm makes for this shape
extern "C" int gptst_stgcn_tapgemm_tpw(int rows, int co, int Ktot, int act) {
    if (rows <= 0 || co <= 0 || Ktot <= 0 || act < 0 || act > 3) return GPTST_EARG;
    return sg_tapgemm_plan(rows, co, Ktot, act).tpw;
}

extern "C" int gptst_stgcn_tapgemm(const float* X, int ldx, int ci, int ntap, int dt0, int dt1, int dt2, int dt3, const float* W, const float* bias,
                                   const float* R, int ldr, int res_w, float* Y, int co, float* S, float* A, int act, int rows, int T, int N,
                                   void* stream) {
    const int dt[4] = {dt0, dt1, dt2, dt3};
    if (!X || !W || !Y || rows <= 0 || T <= 0 || N <= 0 || rows % (T * N) != 0 || ldx < ci || (res_w > 0 && (!R || ldr < res_w)) || res_w > co
        || (S != nullptr) != (A != nullptr) || (S != nullptr && act != SG_ACT_GLU) || act < 0 || act > 3 || !sg_taps_ok(ntap, dt, T))
        return GPTST_EARG;
    const int Ktot = ntap * ci;
    if (ci < 16 || ci % 16 || co < 16 || co % 16 || ldx % 4 || Ktot > 1024) return GPTST_ESHAPE;
    const RowGemmPlan pl = sg_tapgemm_plan(rows, co, Ktot, act);
    const int colblocks = pl.colblocks, rowblocks = pl.rowblocks, tpw = pl.tpw;
    const size_t smem = ((size_t)pl.ocw * (Ktot + 4) + pl.ocw) * sizeof(float);
    SgTg p{X, ldx, ci, SgTap{ntap, {dt0, dt1, dt2, dt3}}, W, Ktot, bias, res_w > 0 ? R : nullptr, ldr, res_w, Y, co, S, A, act, rows, T, N, tpw};
    // more than 64 KB of dynamic LDS needs the attribute, on every device this process launches on
    static bool attr_set[SG_MAX_DEVICES] = {};
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0) return GPTST_EARG;
    if (dev >= SG_MAX_DEVICES || !attr_set[dev]) {
        hipError_t e = hipFuncSetAttribute((const void*)sg_tapgemm_kernel<4>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)((64 * 388 + 64) * sizeof(float)));
        if (e == hipSuccess)
            e = hipFuncSetAttribute((const void*)sg_tapgemm_kernel<2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)((32 * 1028 + 32) * sizeof(float)));
        if (e != hipSuccess) return (int)e;
        if (dev < SG_MAX_DEVICES) attr_set[dev] = true;       // (a race sets it twice: harmless)
    }
    if (pl.wide) hipLaunchKernelGGL(sg_tapgemm_kernel<4>, dim3(rowblocks, colblocks), dim3(ROW_GEMM_THREADS), smem, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(sg_tapgemm_kernel<2>, dim3(rowblocks, colblocks), dim3(ROW_GEMM_THREADS), smem, (hipStream_t)stream, p);
    GPTST_CHECK_LAUNCH();
    return GPTST_OK;
}

extern "C" int gptst_stgcn_gate_bwd(const float* dOut, const float* out, const float* S, const float* A, float* dPre, int act, int rows, int co,
                                    void* stream) {
    if (!dOut || !dPre || rows <= 0 || co <= 0 || act < 1 || act > 3 || (act == SG_ACT_GLU ? (!S || !A) : !out)) return GPTST_EARG;
    if (co % 4) return GPTST_ESHAPE;
    const long n4 = (long)rows * co / 4;
    long blocks = (n4 + 255) / 256; if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(sg_gate_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, dOut, out, S, A, dPre, act, n4, co / 4);
    GPTST_CHECK_LAUNCH();
    return GPTST_OK;
}

extern "C" int gptst_stgcn_wgrad_nsplit(int rows, int cw, int Ktot) {
    if (rows <= 0 || cw <= 0 || Ktot <= 0) return GPTST_EARG;
    return wgrad_split_rule(((cw + 63) / 64) * ((Ktot + 63) / 64), (rows + 63) / 64);
}

extern "C" int gptst_stgcn_wgrad(const float* D, int cw, const float* X, int ldx, int ci, int ntap, int dt0, int dt1, int dt2, int dt3, float* part,
                                 float* bpart, int nsplit, int rows, int T, int N, void* stream) {
    const int dt[4] = {dt0, dt1, dt2, dt3};
    if (!D || !X || !part || rows <= 0 || T <= 0 || N <= 0 || rows % (T * N) != 0 || ldx < ci || !sg_taps_ok(ntap, dt, T)) return GPTST_EARG;
    if (ci < 16 || ci % 16 || cw < 16 || cw % 16 || ldx % 4) return GPTST_ESHAPE;
    const int Ktot = ntap * ci;
    if (nsplit != gptst_stgcn_wgrad_nsplit(rows, cw, Ktot)) return GPTST_EARG;
    const int nchunks = (rows + 63) / 64, cps = (nchunks + nsplit - 1) / nsplit;
    SgWg p{D, cw, X, ldx, ci, SgTap{ntap, {dt0, dt1, dt2, dt3}}, Ktot, part, bpart, rows, T, N, cps, nchunks};
    hipLaunchKernelGGL(sg_wgrad_kernel, dim3((Ktot + 63) / 64, (cw + 63) / 64, nsplit), dim3(256), 0, (hipStream_t)stream, p);
    GPTST_CHECK_LAUNCH();
    return GPTST_OK;
}

extern "C" int gptst_stgcn_nodemix(const float* L, int Np, int ks, const float* In, float* Out, const float* R, int c, int reduce, int units, int N,
                                   void* stream) {
    if (!L || !In || !Out || units <= 0 || N <= 0 || ks <= 0 || (R != nullptr && !reduce)) return GPTST_EARG;
    if (Np != 16 * ((N + 15) / 16) || c < 16 || c % 16 || (size_t)Np * NODE_MIX_P * sizeof(float) > 160 * 1024) return GPTST_ESHAPE;
    const size_t smem = (size_t)Np * NODE_MIX_P * sizeof(float);
    if (smem > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute((const void*)sg_nodemix_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
        if (e != hipSuccess) return (int)e;
    }
    SgNm p{L, Np, ks, In, Out, R, c, reduce, N};
    hipLaunchKernelGGL(sg_nodemix_kernel, dim3(units, (Np / 16 + 3) / 4), dim3(256), smem, (hipStream_t)stream, p);
    GPTST_CHECK_LAUNCH();
    return GPTST_OK;
}

extern "C" int gptst_stgcn_ln_fwd(const float* X, const float* gamma, const float* beta, float* Y, float* mean, float* rstd, int units, int M,
                                  float eps, void* stream) {
    if (!X || !gamma || !beta || !Y || units <= 0 || M <= 0 || (mean != nullptr) != (rstd != nullptr)) return GPTST_EARG;
    if (M % 4) return GPTST_ESHAPE;
    hipLaunchKernelGGL(sg_ln_fwd_kernel, dim3(units), dim3(256), 0, (hipStream_t)stream, X, gamma, beta, Y, mean, rstd, M, eps);
    GPTST_CHECK_LAUNCH();
    return GPTST_OK;
}

extern "C" int gptst_stgcn_ln_bwd(const float* dY, const float* X, const float* gamma, const float* mean, const float* rstd, float* dX, int units,
                                  int M, void* stream) {
    if (!dY || !X || !gamma || !mean || !rstd || !dX || units <= 0 || M <= 0) return GPTST_EARG;
    if (M % 4) return GPTST_ESHAPE;
    hipLaunchKernelGGL(sg_ln_bwd_kernel, dim3(units), dim3(256), 0, (hipStream_t)stream, dY, X, gamma, mean, rstd, dX, M);
    GPTST_CHECK_LAUNCH();
    return GPTST_OK;
}

extern "C" int gptst_stgcn_ln_nsplit(int units) {
    if (units <= 0) return GPTST_EARG;
    const int ups = (units + 15) / 16;
    return (units + ups - 1) / ups;
}

extern "C" int gptst_stgcn_ln_bwd_param(const float* dY, const float* X, const float* mean, const float* rstd, float* pg, float* pb, int nsplit,
                                        int units, int M, void* stream) {
    if (!dY || !X || !mean || !rstd || !pg || !pb || units <= 0 || M <= 0 || nsplit != gptst_stgcn_ln_nsplit(units)) return GPTST_EARG;
    const int ups = (units + nsplit - 1) / nsplit;
    hipLaunchKernelGGL(sg_ln_bwd_param_kernel, dim3((M + 255) / 256, nsplit), dim3(256), 0, (hipStream_t)stream, dY, X, mean, rstd, pg, pb, units, M, ups);
    GPTST_CHECK_LAUNCH();
    return GPTST_OK;
}
