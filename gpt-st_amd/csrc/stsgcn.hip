// The downstream STSGCN predictor (reference model/STSGCN/STSGCN.py; gpt-st_amd/predictors/stsgcn.py) on HIP, forward and backward.
// Channels last, nothing is permuted.  A layer over T frames has W = T - 2 windows of three frames; three row layouts occur:
//   frames     (b, t, n)       (B T N rows)      the layer's input, and the gradient that leaves it
//   expanded   (b, w, k, n)    (B W 3 N rows)    block (w, k), k = 0..2, stands for frame w + k of window w
//   middle     (b, w, n)       (B W N rows)      the last operation's output and the running max: already the next layer's frames
// The STFGNN predictor (stfgnn.hip) has windows of four frames: its expanded rows are groups of R = 4N, which wingemm, gate_bwd and winwgrad
// take as they take 3N — the middle block is rows N .. 2N of a group either way.
//
//   mix        the localized adjacency of a window without its (3N, 3N) matrix: with A^ = the adjacency with a unit diagonal,
//                  mix(S)_k = A^ S_k + [k >= 1] S_{k-1} + [k <= 1] S_{k+1}
//              in five forms.  Forward: frames -> expanded (A^ H_t is formed once per frame and serves the up to three blocks with
//              w + k = t; no expanded copy of the input exists), expanded -> expanded, expanded -> middle (the last operation needs only
//              k = 1).  Adjoints, called with A^T: expanded -> expanded (the same expression), middle -> expanded (blocks 0 and 2 take
//              the gradient unmixed), expanded -> frames (frame t gathers the blocks with w + k = t, in the order k = 0, 1, 2, before
//              the product, and its neighbour terms after it).  Each form is a plan (ss_plan below) that win_mix_body (win_mix_dev.h)
//              runs: the body sf_mix_kernel (stfgnn.hip) runs too, with plans of its own.
//   wingemm    grouped GEMM: row (b, w, ., n) multiplies the weight of window w (stacked (W, cw, ci); one for all: stride 0).  A 16-row
//              tile never straddles two windows: tiles are counted inside each (b, w) group.  Epilogue GLU (S = sigma(Q) and A = P + b
//              kept when asked) or none; on the middle block the GLU epilogue also updates the running max `best` and the winner
//              index `which`: operation 0 writes, later ones replace on strictly greater.  The staging of the window's weight rows is
//              row_gemm_stage (row_gemm_dev.h), shared with sg_tapgemm_kernel (stgcn.hip), and so is the launch plan; the tile loop and
//              the epilogue are this kernel's own.
//   gate_bwd   dPre of operation j = ([upstream] + dBest [which == j] on the middle block) through the GLU derivative (glu_bwd_store)
//   winwgrad   dW (W, cw, ci), db (W, cw) per window: tap_wgrad_body (tap_wgrad_dev.h) with a row map that walks one window's rows
//
// fp32 MFMA 16x16x4 throughout (exact fp32).  Plain launches only: no workgroup waits on another, nothing is accumulated with float atomics.
// No launch asks for more than the 64 KB of dynamic LDS a launch gets by default: the mix serves N <= 448.
#include "common.h"
#include "gptst_hip.h"
#include "row_gemm_dev.h"
#include "tap_wgrad_dev.h"
#include "win_mix_dev.h"

#define SS_ACT_NONE 0
#define SS_ACT_GLU 3

// ---- the mix --------------------------------------------------------------------------------------------------------------------------
struct SsMix { const float* L; int Np; const float* In; float* Out; int c; int mode; int T; int N; };

// what a workgroup's unit does (WinMixPlan, win_mix_dev.h): one phase, slab = sum of up to three source blocks; up to three outputs, each
// [useacc[o]] L slab + the sum of up to four blocks of In
using SsPlan = WinMixPlan<1, 3, 3, 4>;

__device__ __forceinline__ void ss_plan(const SsMix& p, int u, SsPlan& q) {
    const int T = p.T, W = p.T - 2;
    const long N = p.N;
    auto frame = [&](int b, int t) { return ((long)b * T + t) * N; };
    auto blk = [&](int b, int w, int k) { return (((long)b * W + w) * 3 + k) * N; };
    auto mid = [&](int b, int w) { return ((long)b * W + w) * N; };
    int& nsrc = q.nsrc[0];
    long (&src)[3] = q.src[0];
    q.gsel[0] = 0; nsrc = q.nout = 0;
    if (p.mode == WIN_MIX_F2E) {
        const int b = u / T, t = u % T;
        src[nsrc++] = frame(b, t);
        for (int k = 0; k < 3; ++k) {
            const int w = t - k;
            if (w < 0 || w >= W) continue;
            const int o = q.nout++;
            int na = 0;
            q.out[o] = blk(b, w, k); q.useacc[o] = 1;
            if (k >= 1) q.add[o][na++] = frame(b, t - 1);
            if (k <= 1) q.add[o][na++] = frame(b, t + 1);
            q.nadd[o] = na;
        }
    } else if (p.mode == WIN_MIX_E2E) {
        const int b = u / (3 * W), w = (u / 3) % W, k = u % 3;
        int na = 0;
        src[nsrc++] = blk(b, w, k);
        q.out[0] = blk(b, w, k); q.useacc[0] = 1; q.nout = 1;
        if (k >= 1) q.add[0][na++] = blk(b, w, k - 1);
        if (k <= 1) q.add[0][na++] = blk(b, w, k + 1);
        q.nadd[0] = na;
    } else if (p.mode == WIN_MIX_E2M) {
        const int b = u / W, w = u % W;
        src[nsrc++] = blk(b, w, 1);
        q.out[0] = mid(b, w); q.useacc[0] = 1; q.nout = 1;
        q.add[0][0] = blk(b, w, 0); q.add[0][1] = blk(b, w, 2); q.nadd[0] = 2;
    } else if (p.mode == WIN_MIX_M2E) {
        const int b = u / W, w = u % W;
        src[nsrc++] = mid(b, w);
        q.nout = 3;
        for (int k = 0; k < 3; ++k) {
            q.out[k] = blk(b, w, k); q.useacc[k] = k == 1; q.nadd[k] = k == 1 ? 0 : 1; q.add[k][0] = mid(b, w);
        }
    } else {                                                    // WIN_MIX_E2F
        const int b = u / T, t = u % T;
        for (int k = 0; k < 3; ++k) {
            const int w = t - k;
            if (w >= 0 && w < W) src[nsrc++] = blk(b, w, k);
        }
        int na = 0;
        q.out[0] = frame(b, t); q.useacc[0] = 1; q.nout = 1;
        if (t < W) q.add[0][na++] = blk(b, t, 1);                           // forward: Z[w, k] took H[w + k - 1] for k >= 1
        if (t - 1 >= 0 && t - 1 < W) q.add[0][na++] = blk(b, t - 1, 2);
        if (t - 1 >= 0 && t - 1 < W) q.add[0][na++] = blk(b, t - 1, 0);     // and H[w + k + 1] for k <= 1
        if (t - 2 >= 0 && t - 2 < W) q.add[0][na++] = blk(b, t - 2, 1);
        q.nadd[0] = na;
    }
}

// a unit's plan by thread 0, then win_mix_body (win_mix_dev.h) runs it: one graph, one phase
__global__ __launch_bounds__(256) void ss_mix_kernel(SsMix p) {
    extern __shared__ __attribute__((aligned(16))) float slab[];            // [Np][NODE_MIX_P]
    __shared__ SsPlan q;
    if (threadIdx.x == 0) ss_plan(p, blockIdx.x, q);
    __syncthreads();
    const float* const graph[2] = {p.L, p.L};
    win_mix_body(q, graph, p.Np, p.N, p.c, p.In, p.Out, slab);
}

// ---- the grouped GEMM -----------------------------------------------------------------------------------------------------------------
struct SsGemm {
    const float* X; int ci; const float* Wt; long wstride; const float* bias; int bstride;
    float* Y; int co; float* S; float* A; int act;
    float* best; int* which; int opj;
    int B, W, R, N, midoff, tpw;
};

// blockIdx.z = the window, whose weight and bias row_gemm_stage (row_gemm_dev.h) stages; a wave owns 16-row tiles of the window's B groups of R
// rows and NCT column tiles of 16.  Tiles are counted inside each (b, w) group, so none straddles two windows.
template <int NCT>
__global__ __launch_bounds__(ROW_GEMM_THREADS) void ss_wingemm_kernel(SsGemm p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int OCW = 16 * NCT, half = OCW / 2;
    const int P = p.ci + 4;
    const float* Wl = smem;                 // [OCW][P]
    const float* bl = Wl + OCW * P;         // [OCW]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, kk = lane >> 4;
    const int w = blockIdx.z;
    const bool glu = p.act == SS_ACT_GLU;
    const int c0 = row_gemm_stage<NCT>(smem, p.Wt + (size_t)w * p.wstride, p.bias != nullptr ? p.bias + (size_t)w * p.bstride : nullptr, p.ci, p.co, glu);
    const int tpg = (p.R + 15) / 16, ntiles = p.B * tpg, nq = p.ci >> 4;
    const int t0 = (blockIdx.x * (ROW_GEMM_THREADS / 64) + wave) * p.tpw, t1 = min(ntiles, t0 + p.tpw);
    for (int t = t0; t < t1; ++t) {
        const int b = t / tpg, ri0 = (t - b * tpg) * 16;
        const size_t gbase = ((size_t)b * p.W + w) * p.R;                   // first row of the (b, w) group
        const bool rv = ri0 + j < p.R;
        const float* xp = p.X + (gbase + ri0 + j) * p.ci + 4 * kk;
        const float* wl = Wl + j * P + 4 * kk;
        f32x4 acc[NCT];
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) acc[ct] = (f32x4){0.f, 0.f, 0.f, 0.f};
        for (int qd = 0; qd < nq; ++qd) {
            const float4 a0 = rv ? ld4(xp + 16 * qd) : f4zero();
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) {
                const float4 bq = ld4(wl + 16 * ct * P + 16 * qd);
                acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.x, bq.x, acc[ct], 0, 0, 0);
                acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.y, bq.y, acc[ct], 0, 0, 0);
                acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.z, bq.z, acc[ct], 0, 0, 0);
                acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.w, bq.w, acc[ct], 0, 0, 0);
            }
        }
        // ---- epilogue in the accumulator layout: reg r = (row ri0 + kk*4 + r of the group, column 16 ct + j) ----
        if (glu) {
#pragma unroll
            for (int ct = 0; ct < NCT / 2; ++ct) {
                const int ch = c0 + 16 * ct + j;
                if (ch >= p.co) continue;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int ri = ri0 + kk * 4 + r;
                    if (ri >= p.R) continue;
                    const size_t e = (gbase + ri) * p.co + ch;
                    const float pv = acc[ct][r] + bl[16 * ct + j];
                    const float s = sigmoidf_(acc[ct + NCT / 2][r] + bl[half + 16 * ct + j]);
                    const float y = pv * s;
                    p.Y[e] = y;
                    if (p.S != nullptr) { p.S[e] = s; p.A[e] = pv; }
                    if (p.best != nullptr && ri >= p.midoff && ri < p.midoff + p.N) {
                        const size_t m = (((size_t)b * p.W + w) * p.N + (ri - p.midoff)) * p.co + ch;
                        if (p.opj == 0 || y > p.best[m]) {                   // an exact tie keeps the earlier operation
                            p.best[m] = y;
                            if (p.which != nullptr) p.which[m] = p.opj;
                        }
                    }
                }
            }
        } else {
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) {
                const int ch = c0 + 16 * ct + j;
                if (ch >= p.co) continue;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int ri = ri0 + kk * 4 + r;
                    if (ri >= p.R) continue;
                    p.Y[(gbase + ri) * p.co + ch] = acc[ct][r] + bl[16 * ct + j];
                }
            }
        }
    }
}

// ---- dPre (rows, 2 co) of operation j: g = [up] + dBest [which == j] on the middle block;  [g S | g A S (1 - S)] ----
__global__ __launch_bounds__(256) void ss_gate_bwd_kernel(const float* __restrict__ up, const float* __restrict__ dBest, const int* __restrict__ which,
                                                          int opj, const float* __restrict__ S, const float* __restrict__ A,
                                                          float* __restrict__ dPre, long n4, int co4, int R, int N, int midoff) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        const long row = i / co4;
        const int c4 = (int)(i - row * co4);
        const long grp = row / R;
        const int ri = (int)(row - grp * R);
        float4 g = up != nullptr ? ld4(up + 4 * i) : f4zero();
        if (ri >= midoff && ri < midoff + N) {
            const long m = ((grp * N + (ri - midoff)) * co4 + c4) * 4;
            const float4 d = ld4(dBest + m);
            const int4 wh = *reinterpret_cast<const int4*>(which + m);
            g.x += wh.x == opj ? d.x : 0.f; g.y += wh.y == opj ? d.y : 0.f; g.z += wh.z == opj ? d.z : 0.f; g.w += wh.w == opj ? d.w : 0.f;
        }
        const float4 s = ld4(S + 4 * i), a = ld4(A + 4 * i);
        glu_bwd_store(dPre + (row * 2 * co4 + c4) * 4, co4, g, s, a);
    }
}

// ---- the weight gradient per window ----
struct SsWgrad { const float* D; int cw; const float* X; int ci; float* part; float* bpart; int B, W, R, ns, cps, nchunks; };

// blockIdx.z = window * ns + split; virtual row v of a window = row v % R of the group (v / R, window)
struct SsWgRows {
    int w, s, W, R, ns;
    __device__ __forceinline__ SsWgRows(const SsWgrad& p) : w(blockIdx.z / p.ns), s(blockIdx.z % p.ns), W(p.W), R(p.R), ns(p.ns) {}
    __device__ __forceinline__ int split() const { return s; }
    __device__ __forceinline__ int slot() const { return w * ns + s; }
    __device__ __forceinline__ size_t operator()(int v) const { const int b = v / R; return ((size_t)b * W + w) * R + (v - b * R); }
};

struct SsWgSrc {
    const SsWgrad& p; const SsWgRows& rows; int kcol; bool kv;
    __device__ __forceinline__ SsWgSrc(const SsWgrad& p_, const SsWgRows& r_, int kcol_) : p(p_), rows(r_), kcol(kcol_), kv(kcol_ < p_.ci) {}
    __device__ __forceinline__ float4 operator()(int v, bool rv) const { return (rv && kv) ? ld4(p.X + rows(v) * p.ci + kcol) : f4zero(); }
};

__global__ __launch_bounds__(256) void ss_winwgrad_kernel(SsWgrad p) {
    const SsWgRows rows(p);
    tap_wgrad_body(p.D, p.cw, p.ci, p.part, p.bpart, p.B * p.R, p.cps, p.nchunks, SsWgSrc(p, rows, blockIdx.x * 64 + 4 * (threadIdx.x & 15)), rows);
}

// ---- entry points ----
extern "C" int gptst_stsgcn_mix(const float* L, int Np, const float* In, float* Out, int c, int mode, int B, int T, int N, void* stream) {
    if (!L || !In || !Out || In == Out || B <= 0 || T < 3 || N <= 0 || mode < 0 || mode > 4) return GPTST_EARG;
    if (Np != 16 * ((N + 15) / 16) || Np > WIN_MIX_MAX_NP || c < 16 || c % 16) return GPTST_ESHAPE;
    const long W = T - 2;
    const long units = mode == WIN_MIX_F2E || mode == WIN_MIX_E2F ? (long)B * T : mode == WIN_MIX_E2E ? (long)B * W * 3 : (long)B * W;
    if (units > 0x7fffffffL) return GPTST_ESHAPE;
    static_assert(WIN_MIX_MAX_NP * NODE_MIX_P * sizeof(float) + sizeof(SsPlan) <= 64 * 1024, "slab + plan exceed the default dynamic LDS");
    const size_t smem = (size_t)Np * NODE_MIX_P * sizeof(float);
    SsMix p{L, Np, In, Out, c, mode, T, N};
    hipLaunchKernelGGL(ss_mix_kernel, dim3((unsigned)units, (Np / 16 + 3) / 4), dim3(256), smem, (hipStream_t)stream, p);
    GPTST_CHECK_LAUNCH();
    return GPTST_OK;
}

// the launch plan of the grouped GEMM: 64 weight rows where they fit the 64 KB a launch gets by default, else 32; about 1024 workgroups over the W windows
static RowGemmPlan ss_wingemm_plan(int B, int W, int R, int ci, int co, int act) {
    const bool wide = ((size_t)64 * (ci + 4) + 64) * sizeof(float) <= 64 * 1024;
    return row_gemm_plan((long)B * ((R + 15) / 16), co, act == SS_ACT_GLU, wide, W, 1024);
}

// (include/gptst_hip_testing.h) tiles per wave of the launch gptst_stsgcn_wingemm makes for this shape
extern "C" int gptst_stsgcn_wingemm_tpw(int B, int W, int R, int ci, int co, int act) {
    if (B <= 0 || W <= 0 || R <= 0 || ci <= 0 || co <= 0 || (act != SS_ACT_NONE && act != SS_ACT_GLU)) return GPTST_EARG;
    return ss_wingemm_plan(B, W, R, ci, co, act).tpw;
}

extern "C" int gptst_stsgcn_wingemm(const float* X, int ci, const float* Wt, const float* bias, int shared, float* Y, int co, float* S, float* A,
                                    int act, float* best, int* which, int opj, int B, int W, int R, int N, void* stream) {
    if (!X || !Wt || !Y || B <= 0 || W <= 0 || N <= 0 || (R != N && R != 3 * N && R != 4 * N) || (S != nullptr) != (A != nullptr)
        || (act != SS_ACT_NONE && act != SS_ACT_GLU) || ((S != nullptr || best != nullptr) && act != SS_ACT_GLU) || (which != nullptr && !best)
        || opj < 0)
        return GPTST_EARG;
    if (ci < 16 || ci % 16 || ci > 256 || co < 16 || co % 16 || W > 65535 || (long)B * ((R + 15) / 16) > 0x7fffffffL) return GPTST_ESHAPE;
    const RowGemmPlan pl = ss_wingemm_plan(B, W, R, ci, co, act);
    const int cw = act == SS_ACT_GLU ? 2 * co : co, colblocks = pl.colblocks, rowblocks = pl.rowblocks;
    if (colblocks > 65535) return GPTST_ESHAPE;
    const size_t smem = ((size_t)pl.ocw * (ci + 4) + pl.ocw) * sizeof(float);
    SsGemm p{X, ci, Wt, shared ? 0L : (long)cw * ci, bias, shared ? 0 : cw, Y, co, S, A, act, best, which, opj, B, W, R, N, R == N ? 0 : N, pl.tpw};
    if (pl.wide) hipLaunchKernelGGL(ss_wingemm_kernel<4>, dim3(rowblocks, colblocks, W), dim3(ROW_GEMM_THREADS), smem, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(ss_wingemm_kernel<2>, dim3(rowblocks, colblocks, W), dim3(ROW_GEMM_THREADS), smem, (hipStream_t)stream, p);
    GPTST_CHECK_LAUNCH();
    return GPTST_OK;
}

extern "C" int gptst_stsgcn_gate_bwd(const float* up, const float* dBest, const int* which, int opj, const float* S, const float* A, float* dPre,
                                     int B, int W, int R, int N, int co, void* stream) {
    if (!dBest || !which || !S || !A || !dPre || B <= 0 || W <= 0 || N <= 0 || (R != N && R != 3 * N && R != 4 * N) || opj < 0) return GPTST_EARG;
    if (co < 4 || co % 4) return GPTST_ESHAPE;
    const long n4 = (long)B * W * R * co / 4;
    long blocks = (n4 + 255) / 256; if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(ss_gate_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, up, dBest, which, opj, S, A, dPre, n4, co / 4, R, N,
                       R == N ? 0 : N);
    GPTST_CHECK_LAUNCH();
    return GPTST_OK;
}

// splits of one window's B R rows
extern "C" int gptst_stsgcn_winwgrad_nsplit(int wrows, int cw, int ci, int W) {
    if (wrows <= 0 || cw <= 0 || ci <= 0 || W <= 0) return GPTST_EARG;
    return wgrad_split_rule(((cw + 63) / 64) * ((ci + 63) / 64) * W, (wrows + 63) / 64);
}

extern "C" int gptst_stsgcn_winwgrad(const float* D, int cw, const float* X, int ci, float* part, float* bpart, int nsplit, int B, int W, int R,
                                     void* stream) {
    if (!D || !X || !part || B <= 0 || W <= 0 || R <= 0 || (long)B * R > 0x7fffffffL) return GPTST_EARG;
    if (ci < 16 || ci % 16 || cw < 16 || cw % 16 || (long)W * nsplit > 65535) return GPTST_ESHAPE;
    if (nsplit != gptst_stsgcn_winwgrad_nsplit(B * R, cw, ci, W)) return GPTST_EARG;
    const int nchunks = (B * R + 63) / 64, cps = (nchunks + nsplit - 1) / nsplit;
    SsWgrad p{D, cw, X, ci, part, bpart, B, W, R, nsplit, cps, nchunks};
    hipLaunchKernelGGL(ss_winwgrad_kernel, dim3((ci + 63) / 64, (cw + 63) / 64, W * nsplit), dim3(256), 0, (hipStream_t)stream, p);
    GPTST_CHECK_LAUNCH();
    return GPTST_OK;
}
