// The downstream MTGNN predictor (reference model/MTGNN/MTGNN.py; gpt-st_amd/predictors/mtgnn.py) on HIP: the kernels the STGCN / TGCN
// families (stgcn.hip, tgcn.hip: both unchanged, and called wherever they serve) do not have.  Channels-last rows (b, t, n) as there; a
// tensor's time length is its FRAME: MTGNN's temporal convolutions are valid ones, so the input frame Tsrc and the output frame Tdst differ.
//
//   tapgemm     Y[b, to, n, :] = epi(sum_j X[b, to + off_j, n, :] W_j + bias): up to 32 taps of any offset (a tap outside [0, Tsrc) is not
//               read), K walked in chunks of 128 through LDS (skip0: K = 20 * 64).  Epilogues: plain, with a residual of its own frame and an
//               output multiplier; or gated, tanh(P) sigmoid(Q) keep (P and Q channels of one output in one lane).  An operand multiplier
//               serves the dropout in front of skip0.  With the taps mirrored and the weights transposed by the caller the same kernel is
//               the data backward (the predicate per row is what a 'full' correlation needs); the residual carries a second gradient in.
//   gate_bwd    dPre = [dG keep s (1 - tn^2) | dG keep tn s (1 - s)] from the kept tanh, sigmoid and keep multiplier
//   wgrad       dW_j = sum X[b, to + off_j]^T dPre and db: row-split partials written whole, summed by the caller in a fixed order
//   graphgrad   dM_k[v, w] = sum_{unit, c} dZ_k[unit, v, c] X[unit, w, c] for ks graphs at once: the gradient of gptst_stgcn_nodemix with
//               respect to its graphs (the adjacency is learned here).  Unit-split partials.  A unit is N rows: rows past N are the next
//               unit's data and are not read.
//
// fp32 MFMA 16x16x4 throughout (exact fp32).  Plain launches only: no workgroup waits on another, nothing is accumulated with float atomics.
#include "common.h"
#include "gptst_hip.h"
#include "tap_wgrad_dev.h"

#define MT_THREADS 256
#define MT_KC 128                  // K chunk of the tap GEMM: 64 weight rows of 128 floats in LDS (33 KB)
#define MT_P (MT_KC + 4)
#define MT_MAX_TAPS 32

struct MtTaps { int n; int off[MT_MAX_TAPS]; };

struct MtTg {
    const float* X; int ldx; int ci; const float* XM; MtTaps tap;
    const float* W; int Ktot; const float* bias;
    const float* R; int ldr; int Tr; int roff;
    const float* OM; float* Y; int co; float* Tn; float* S; int gated;
    int rows, Tsrc, Tdst, N;
};

// a wave owns TPW 16-row tiles and four column tiles of 16; the workgroup's 64 weight rows of the current K chunk sit in LDS.  Gated: column
// tiles 0, 1 are the filter (P) channels and 2, 3 the gate (Q) channels of the same 32 outputs, so a lane holds P and Q of one (row, channel).
template <int TPW>
__global__ __launch_bounds__(MT_THREADS) void mt_tapgemm_kernel(MtTg p) {
    __shared__ __attribute__((aligned(16))) float Wl[64 * MT_P];
    __shared__ float bl[64];
    __shared__ int offl[MT_MAX_TAPS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, kk = lane >> 4;
    const int c0 = blockIdx.y * (p.gated ? 32 : 64);
    if (tid < 64) {
        const int ch = p.gated ? c0 + (tid & 31) : c0 + tid;
        const int wr = (p.gated && tid >= 32) ? p.co + ch : ch;
        bl[tid] = (p.bias != nullptr && ch < p.co) ? p.bias[wr] : 0.f;
    } else if (tid < 64 + MT_MAX_TAPS) {
        offl[tid - 64] = tid - 64 < p.tap.n ? p.tap.off[tid - 64] : 0;
    }
    const int tile0 = (blockIdx.x * (MT_THREADS / 64) + wave) * TPW;
    long src[TPW];                                  // this lane's A row in the source frame at offset 0
    int tdst[TPW];
    bool rv[TPW];
#pragma unroll
    for (int i = 0; i < TPW; ++i) {
        const int ra = (tile0 + i) * 16 + j;
        rv[i] = ra < p.rows;
        const int n = ra % p.N, bt = ra / p.N;
        tdst[i] = bt % p.Tdst;
        src[i] = ((long)(bt / p.Tdst) * p.Tsrc + tdst[i]) * p.N + n;
    }
    f32x4 acc[TPW][4];
#pragma unroll
    for (int i = 0; i < TPW; ++i)
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) acc[i][ct] = (f32x4){0.f, 0.f, 0.f, 0.f};
    __syncthreads();                                // bl, offl are written
    for (int k0 = 0; k0 < p.Ktot; k0 += MT_KC) {
        const int kc = min(MT_KC, p.Ktot - k0), k4 = kc >> 2;
        // does any row of this workgroup read a tap of this chunk?  Always, in a valid convolution; in the data backward of a whole-axis
        // contraction a row reads ONE tap of up to 32, and a workgroup's rows span two time steps at the most
        bool need = false;
        for (int tp = k0 / p.ci; tp <= (k0 + kc - 1) / p.ci; ++tp) {
#pragma unroll
            for (int i = 0; i < TPW; ++i) { const int ts = tdst[i] + offl[tp]; need |= rv[i] && ts >= 0 && ts < p.Tsrc; }
        }
        if (!__syncthreads_or(need)) continue;      // (the barrier: the previous chunk's reads of Wl are done)
        for (int f = tid; f < 64 * k4; f += MT_THREADS) {
            const int l = f / k4, c4 = f - l * k4;
            const int ch = p.gated ? c0 + (l & 31) : c0 + l;
            const int wr = (p.gated && l >= 32) ? p.co + ch : ch;
            st4(Wl + l * MT_P + 4 * c4, ch < p.co ? ld4(p.W + (size_t)wr * p.Ktot + k0 + 4 * c4) : f4zero());
        }
        __syncthreads();
        for (int g = 0; g < (kc >> 4); ++g) {
            const int k = k0 + 16 * g, tp = k / p.ci, xc = k - tp * p.ci, off = offl[tp];
            bool ok[TPW], any = false;
#pragma unroll
            for (int i = 0; i < TPW; ++i) {
                const int ts = tdst[i] + off;
                ok[i] = rv[i] && ts >= 0 && ts < p.Tsrc;              // a tap outside the source frame contributes nothing and is not loaded
                any |= ok[i];
            }
            if (!__any(any)) continue;                                // no row of this wave reads this tap
            float4 a[TPW];
#pragma unroll
            for (int i = 0; i < TPW; ++i) {
                const long e = (src[i] + (long)off * p.N) * p.ldx + xc + 4 * kk;
                a[i] = ok[i] ? ld4(p.X + e) : f4zero();
                if (p.XM != nullptr && ok[i]) { const float4 m = ld4(p.XM + e); a[i] = make_float4(a[i].x * m.x, a[i].y * m.y, a[i].z * m.z, a[i].w * m.w); }
            }
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) {
                const float4 b = ld4(Wl + (16 * ct + j) * MT_P + 16 * g + 4 * kk);
#pragma unroll
                for (int i = 0; i < TPW; ++i) {
                    acc[i][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i].x, b.x, acc[i][ct], 0, 0, 0);
                    acc[i][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i].y, b.y, acc[i][ct], 0, 0, 0);
                    acc[i][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i].z, b.z, acc[i][ct], 0, 0, 0);
                    acc[i][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i].w, b.w, acc[i][ct], 0, 0, 0);
                }
            }
        }
    }
    // ---- epilogue in the accumulator layout: reg r = (row kk*4 + r, column 16 ct + j) ----
#pragma unroll
    for (int i = 0; i < TPW; ++i) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = (tile0 + i) * 16 + kk * 4 + r;
            if (row >= p.rows) continue;
            if (p.gated) {
#pragma unroll
                for (int ct = 0; ct < 2; ++ct) {
                    const int ch = c0 + 16 * ct + j;
                    if (ch >= p.co) continue;
                    const float tn = tanhf(acc[i][ct][r] + bl[16 * ct + j]);
                    const float s = sigmoidf_(acc[i][ct + 2][r] + bl[32 + 16 * ct + j]);
                    const size_t o = (size_t)row * p.co + ch;
                    p.Y[o] = p.OM != nullptr ? tn * s * p.OM[o] : tn * s;
                    if (p.Tn != nullptr) { p.Tn[o] = tn; p.S[o] = s; }
                }
            } else {
                long rr = -1;                        // the residual's row: its own frame, Tr long, read at to + roff when that is inside
                if (p.R != nullptr) {
                    const int n = row % p.N, bt = row / p.N, tr = bt % p.Tdst + p.roff;
                    if (tr >= 0 && tr < p.Tr) rr = ((long)(bt / p.Tdst) * p.Tr + tr) * p.N + n;
                }
#pragma unroll
                for (int ct = 0; ct < 4; ++ct) {
                    const int ch = c0 + 16 * ct + j;
                    if (ch >= p.co) continue;
                    float v = acc[i][ct][r] + bl[16 * ct + j];
                    if (rr >= 0) v += p.R[rr * p.ldr + ch];
                    const size_t o = (size_t)row * p.co + ch;
                    p.Y[o] = p.OM != nullptr ? v * p.OM[o] : v;
                }
            }
        }
    }
}

// dPre (rows, 2 co) = [dG keep s (1 - tn^2) | dG keep tn s (1 - s)]   (g = tanh(P) sigmoid(Q) keep; keep = NULL: 1)
__global__ __launch_bounds__(256) void mt_gate_bwd_kernel(const float* __restrict__ dG, const float* __restrict__ Tn, const float* __restrict__ S,
                                                          const float* __restrict__ OM, float* __restrict__ dPre, long n4, int co4) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        float4 g = ld4(dG + 4 * i);
        if (OM != nullptr) { const float4 m = ld4(OM + 4 * i); g = make_float4(g.x * m.x, g.y * m.y, g.z * m.z, g.w * m.w); }
        const float4 t = ld4(Tn + 4 * i), s = ld4(S + 4 * i);
        const long row = i / co4;
        const int c4 = (int)(i - row * co4);
        float* d = dPre + (row * 2 * co4 + c4) * 4;
        st4(d, make_float4(g.x * s.x * (1.f - t.x * t.x), g.y * s.y * (1.f - t.y * t.y), g.z * s.z * (1.f - t.z * t.z), g.w * s.w * (1.f - t.w * t.w)));
        st4(d + 4 * co4, make_float4(g.x * t.x * (s.x * (1.f - s.x)), g.y * t.y * (s.y * (1.f - s.y)), g.z * t.z * (s.z * (1.f - s.z)),
                                     g.w * t.w * (s.w * (1.f - s.w))));
    }
}

// ---- weight gradient: part[z][o][k] = sum over the rows of split z of D[row][o] X[row's source row at tap(k)][k mod ci]; bpart[z][o] = column
// sums of D.  D is in the destination frame, X in the source frame (sg_wgrad_kernel with the two frames and the tap table). ----
struct MtWg {
    const float* D; int cw; const float* X; int ldx; int ci; const float* XM; MtTaps tap; int Ktot;
    float* part; float* bpart; int rows, Tsrc, Tdst, N, cps, nchunks;
};

// the source of a destination row for this thread's columns: the same (b, n) at to + off in the source frame, times its mask
struct MtWgSrc {
    const MtWg& p; bool kv; int xc, off;
    __device__ __forceinline__ MtWgSrc(const MtWg& p_, int kcol) : p(p_), kv(kcol < p_.Ktot) {
        const int tp = kv ? kcol / p.ci : 0;
        xc = kcol - tp * p.ci; off = p.tap.off[tp];
    }
    __device__ __forceinline__ float4 operator()(int row, bool rv) const {
        const int n = row % p.N, bt = row / p.N, ts = bt % p.Tdst + off;
        float4 x = f4zero();
        if (rv && kv && ts >= 0 && ts < p.Tsrc) {
            const long e = (((long)(bt / p.Tdst) * p.Tsrc + ts) * p.N + n) * p.ldx + xc;
            x = ld4(p.X + e);
            if (p.XM != nullptr) { const float4 m = ld4(p.XM + e); x = make_float4(x.x * m.x, x.y * m.y, x.z * m.z, x.w * m.w); }
        }
        return x;
    }
};

__global__ __launch_bounds__(256) void mt_wgrad_kernel(MtWg p) {
    tap_wgrad_body(p.D, p.cw, p.Ktot, p.part, p.bpart, p.rows, p.cps, p.nchunks, MtWgSrc(p, blockIdx.x * 64 + 4 * (threadIdx.x & 15)));
}

// ---- gradient of the node mix with respect to its graphs: a 64 x 64 tile of dM_k per workgroup, 32 channels of one unit per stage ----
#define MT_GG_P 36

struct MtGg { const float* D; int ldd; int dcol0; const float* X; int ldx; int c; int ks; float* part; int units, N, ups, tw; };

__global__ __launch_bounds__(256) void mt_graphgrad_kernel(MtGg p) {
    __shared__ __attribute__((aligned(16))) float Dl[64 * MT_GG_P];
    __shared__ __attribute__((aligned(16))) float Xl[64 * MT_GG_P];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, kk = lane >> 4;
    const int v0 = (blockIdx.x / p.tw) * 64, w0 = (blockIdx.x % p.tw) * 64, k = blockIdx.y, z = blockIdx.z;
    const int u0 = z * p.ups, u1 = min(p.units, u0 + p.ups);
    const int ncg = (p.c + 31) / 32, steps = (u1 - u0) * ncg;
    const int c4 = tid & 7, rb = tid >> 3;                  // this thread's two float4 of either tile: rows rb and rb + 32, columns 4 c4
    f32x4 acc[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) acc[nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float4 dr[2], xr[2];
    auto fetch = [&](int step) {
        const int unit = u0 + step / ncg, cc = 32 * (step % ncg) + 4 * c4;
        const size_t base = (size_t)unit * p.N;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int v = v0 + rb + 32 * i, w = w0 + rb + 32 * i;      // a node past N is the next unit's row: not read
            dr[i] = (v < p.N && cc < p.c) ? ld4(p.D + (base + v) * p.ldd + p.dcol0 + k * p.c + cc) : f4zero();
            xr[i] = (w < p.N && cc < p.c) ? ld4(p.X + (base + w) * p.ldx + cc) : f4zero();
        }
    };
    if (steps > 0) fetch(0);
    for (int step = 0; step < steps; ++step) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 2; ++i) { st4(Dl + (rb + 32 * i) * MT_GG_P + 4 * c4, dr[i]); st4(Xl + (rb + 32 * i) * MT_GG_P + 4 * c4, xr[i]); }
        __syncthreads();
        if (step + 1 < steps) fetch(step + 1);
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const float4 a = ld4(Dl + (16 * wave + j) * MT_GG_P + 16 * q + 4 * kk);
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                const float4 b = ld4(Xl + (16 * nt + j) * MT_GG_P + 16 * q + 4 * kk);
                acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc[nt], 0, 0, 0);
                acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc[nt], 0, 0, 0);
                acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc[nt], 0, 0, 0);
                acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc[nt], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        const int w = w0 + 16 * nt + j;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int v = v0 + 16 * wave + kk * 4 + r;
            if (v < p.N && w < p.N) p.part[(((size_t)z * p.ks + k) * p.N + v) * p.N + w] = acc[nt][r];
        }
    }
}

// ---- entry points ----
static bool mt_taps(MtTaps& t, int ntap, const int* offs, int Tsrc, int Tdst) {
    if (ntap < 1 || ntap > MT_MAX_TAPS || offs == nullptr) return false;
    t.n = ntap;
    for (int i = 0; i < MT_MAX_TAPS; ++i) t.off[i] = i < ntap ? offs[i] : 0;
    for (int i = 0; i < ntap; ++i) if (offs[i] <= -Tdst || offs[i] >= Tsrc) return false;     // (such a tap would touch no row at all)
    return true;
}

// the launch plan of the tap GEMM: the one place that derives it, for the launch and for the query of the tests
struct MtTgPlan { int colblocks, rowblocks, tpw; };

static MtTgPlan mt_tapgemm_plan(long rows, int co, int gated) {
    MtTgPlan g;
    const int per = gated ? 32 : 64, ntiles = (int)((rows + 15) / 16), wpb = MT_THREADS / 64;
    g.colblocks = (co + per - 1) / per;
    const bool two = (ntiles + 2 * wpb - 1) / (2 * wpb) * g.colblocks >= 512;    // two tiles per wave once that still fills the device twice
    g.tpw = two ? 2 : 1;
    g.rowblocks = (ntiles + wpb * g.tpw - 1) / (wpb * g.tpw);
    return g;
}

// (include/gptst_hip_testing.h) tiles per wave of the launch gptst_mtgnn_tapgemm makes for this shape: 1 or 2
extern "C" int gptst_mtgnn_tapgemm_tpw(long rows, int co, int gated) {
    if (rows <= 0 || rows > (1L << 30) || co <= 0) return GPTST_EARG;
    return mt_tapgemm_plan(rows, co, gated).tpw;
}

extern "C" int gptst_mtgnn_tapgemm(const float* X, int ldx, int ci, const float* XM, int ntap, const int* offs, const float* W, const float* bias,
                                   const float* R, int ldr, int Tr, int roff, const float* OM, float* Y, int co, float* Tn, float* S, int gated,
                                   int B, int Tsrc, int Tdst, int N, void* stream) {
    MtTaps tap;
    if (!X || !W || !Y || B <= 0 || Tsrc <= 0 || Tdst <= 0 || N <= 0 || ldx < ci || (R != nullptr && (ldr < co || Tr <= 0 || gated))
        || (Tn != nullptr) != (S != nullptr) || (Tn != nullptr && !gated) || !mt_taps(tap, ntap, offs, Tsrc, Tdst))
        return GPTST_EARG;
    const long rows = (long)B * Tdst * N;
    if (ci < 16 || ci % 16 || co < 16 || co % 16 || ldx % 4 || rows > (1L << 30) || (long)B * Tsrc * N > (1L << 30)) return GPTST_ESHAPE;
    const MtTgPlan g = mt_tapgemm_plan(rows, co, gated);
    const bool two = g.tpw == 2;
    const int colblocks = g.colblocks, rowblocks = g.rowblocks;
    MtTg p{X, ldx, ci, XM, tap, W, ntap * ci, bias, R, ldr, Tr, roff, OM, Y, co, Tn, S, gated, (int)rows, Tsrc, Tdst, N};
    if (two) hipLaunchKernelGGL(mt_tapgemm_kernel<2>, dim3(rowblocks, colblocks), dim3(MT_THREADS), 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(mt_tapgemm_kernel<1>, dim3(rowblocks, colblocks), dim3(MT_THREADS), 0, (hipStream_t)stream, p);
    GPTST_CHECK_LAUNCH();
    return GPTST_OK;
}

extern "C" int gptst_mtgnn_gate_bwd(const float* dG, const float* Tn, const float* S, const float* OM, float* dPre, int rows, int co, void* stream) {
    if (!dG || !Tn || !S || !dPre || rows <= 0 || co <= 0) return GPTST_EARG;
    if (co % 4) return GPTST_ESHAPE;
    const long n4 = (long)rows * co / 4;
    long blocks = (n4 + 255) / 256; if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(mt_gate_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, dG, Tn, S, OM, dPre, n4, co / 4);
    GPTST_CHECK_LAUNCH();
    return GPTST_OK;
}

extern "C" int gptst_mtgnn_wgrad(const float* D, int cw, const float* X, int ldx, int ci, const float* XM, int ntap, const int* offs, float* part,
                                 float* bpart, int nsplit, int B, int Tsrc, int Tdst, int N, void* stream) {
    MtTaps tap;
    if (!D || !X || !part || B <= 0 || Tsrc <= 0 || Tdst <= 0 || N <= 0 || ldx < ci || !mt_taps(tap, ntap, offs, Tsrc, Tdst)) return GPTST_EARG;
    const long rows = (long)B * Tdst * N;
    if (ci < 16 || ci % 16 || cw < 16 || cw % 16 || ldx % 4 || rows > (1L << 30) || (long)B * Tsrc * N > (1L << 30)) return GPTST_ESHAPE;
    const int Ktot = ntap * ci;
    if (nsplit != gptst_stgcn_wgrad_nsplit((int)rows, cw, Ktot)) return GPTST_EARG;      // the same split rule as the STGCN weight gradient
    const int nchunks = (int)((rows + 63) / 64), cps = (nchunks + nsplit - 1) / nsplit;
    MtWg p{D, cw, X, ldx, ci, XM, tap, Ktot, part, bpart, (int)rows, Tsrc, Tdst, N, cps, nchunks};
    hipLaunchKernelGGL(mt_wgrad_kernel, dim3((Ktot + 63) / 64, (cw + 63) / 64, nsplit), dim3(256), 0, (hipStream_t)stream, p);
    GPTST_CHECK_LAUNCH();
    return GPTST_OK;
}

extern "C" int gptst_mtgnn_graphgrad_nsplit(int units, int N, int ks) {
    if (units <= 0 || N <= 0 || ks <= 0) return GPTST_EARG;
    const int t = (N + 63) / 64;
    return wgrad_split_rule(t * t * ks, units);
}

extern "C" int gptst_mtgnn_graphgrad(const float* D, int ldd, int dcol0, const float* X, int ldx, int c, int ks, float* part, int nsplit, int units,
                                     int N, void* stream) {
    if (!D || !X || !part || units <= 0 || N <= 0 || ks <= 0 || dcol0 < 0 || ldd < dcol0 + ks * c || ldx < c
        || nsplit != gptst_mtgnn_graphgrad_nsplit(units, N, ks))
        return GPTST_EARG;
    if (c < 16 || c % 16 || ldd % 4 || ldx % 4 || dcol0 % 4 || ks > 65535 || (long)units * N > (1L << 30)) return GPTST_ESHAPE;
    const int t = (N + 63) / 64, ups = (units + nsplit - 1) / nsplit;
    MtGg p{D, ldd, dcol0, X, ldx, c, ks, part, units, N, ups, t};
    hipLaunchKernelGGL(mt_graphgrad_kernel, dim3(t * t, ks, nsplit), dim3(256), 0, (hipStream_t)stream, p);
    GPTST_CHECK_LAUNCH();
    return GPTST_OK;
}
