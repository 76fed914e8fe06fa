// The fusion-graph product of the downstream STFGNN predictor (reference model/STFGNN/STFGNN.py; gpt-st_amd/predictors/stfgnn.py) on HIP.
// A layer over T frames has W = T - 3 windows of four frames; the row layouts are those of stsgcn.hip with four blocks:
//   frames     (b, t, n)       (B T N rows)      the layer's input, and the gradient that leaves it
//   expanded   (b, w, k, n)    (B W 4 N rows)    block (w, k), k = 0..3, stands for frame w + k of window w
//   middle     (b, w, n)       (B W N rows)      the last operation's output and the running max: already the next layer's frames
//
// The (4N, 4N) spatial-temporal fusion graph (construct_adj_fusion) is, with S^ the spatial adjacency with a unit diagonal, D the temporal
// (DTW) graph, which has one, and 1 the identity block,
//        [ D 1  1  D ]
//        [ 1 S^ 1  1 ]       so for a source X of four blocks   mix(X)_0 = mix(X)_3 = D (X_0 + X_3) + X_1 + X_2
//        [ 1 1  S^ 1 ]                                          mix(X)_1 = S^ X_1 + X_0 + X_2 + X_3
//        [ D 1  1  D ]                                          mix(X)_2 = S^ X_2 + X_0 + X_1 + X_3
// three N x N products per window, the matrix never formed.  A workgroup's unit is a plan: up to two phases, each the product of one of the
// two graphs with a slab that is the sum of up to four source blocks, both added into the same accumulators; then up to four output blocks,
// each the accumulator (or nothing) plus up to ten blocks of the input unmixed.  The five forms:
//   F2E  frames -> expanded.  B T units "S^ H_t", formed once per frame and written to the blocks k = 1, 2 of the windows that hold it, and
//        B W units "D (H_w + H_{w+3})", formed once per window and written to BOTH blocks 0 and 3.  No expanded copy of the input exists.
//   E2E  expanded -> expanded, three units per window; the outer one has the slab X_0 + X_3 and two outputs.  Called with S^T and D^T it is
//        its own adjoint (the transposed matrix has the same form).
//   E2M  expanded -> middle: block 1 only, S^ only (the last operation of a layer is cropped to it).
//   M2E  the adjoint of E2M (called with S^T): block 1 takes the product, blocks 0, 2 and 3 the gradient unmixed.
//   E2F  the adjoint of F2E (called with S^T, D^T): frame t is the sum of two slab products, done in ONE workgroup one after the other —
//        phase 0:  S^T (G[t-1, 1] + G[t-2, 2]),  phase 1:  D^T (G[t, 0] + G[t, 3] + G[t-3, 0] + G[t-3, 3])  (blocks gathered in this order) —
//        plus the unmixed blocks, in this order:  G[t-1, 0], G[t-1, 3], G[t-2, 0], G[t-2, 3], G[t, 1], G[t-2, 1], G[t-3, 1], G[t, 2], G[t-1, 2],
//        G[t-3, 2]; every block whose window exists.
// sf_plan below writes the plan of a unit; what runs it is win_mix_body (win_mix_dev.h), the body ss_mix_kernel (stsgcn.hip) runs with its
// one-phase plans.
//
// fp32 MFMA 16x16x4 (exact fp32).  Plain launches only: no workgroup waits on another, nothing is accumulated with float atomics, the order of
// every sum is fixed.  No launch asks for more than the 64 KB of dynamic LDS a launch gets by default: N <= 448 (GPTST_ESHAPE beyond).
#include "common.h"
#include "gptst_hip.h"
#include "win_mix_dev.h"

struct SfMix { const float* S; const float* D; int Np; const float* In; float* Out; int c; int mode; int B; int T; int N; };

// what a workgroup's unit does (WinMixPlan, win_mix_dev.h): up to two phases of up to four source blocks, up to four outputs of up to ten adds;
// a phase without sources is skipped
using SfPlan = WinMixPlan<2, 4, 4, 10>;

__device__ __forceinline__ void sf_plan(const SfMix& p, int u, SfPlan& q) {
    const int T = p.T, W = p.T - 3;
    const long N = p.N;
    auto frame = [&](int b, int t) { return ((long)b * T + t) * N; };
    auto blk = [&](int b, int w, int k) { return (((long)b * W + w) * 4 + k) * N; };
    auto mid = [&](int b, int w) { return ((long)b * W + w) * N; };
    auto win = [&](int w) { return w >= 0 && w < W; };
    q.nout = 0;
    q.gsel[0] = q.gsel[1] = 0; q.nsrc[0] = q.nsrc[1] = 0;
    if (p.mode == WIN_MIX_F2E) {
        if (u < p.B * T) {                                          // S^ H_t -> the blocks k = 1, 2 with w + k = t
            const int b = u / T, t = u % T;
            q.src[0][q.nsrc[0]++] = frame(b, t);
            for (int k = 1; k <= 2; ++k) {
                const int w = t - k;
                if (!win(w)) continue;
                const int o = q.nout++;
                int na = 0;
                q.out[o] = blk(b, w, k); q.useacc[o] = 1;
                for (int k2 = 0; k2 < 4; ++k2)
                    if (k2 != k) q.add[o][na++] = frame(b, w + k2);
                q.nadd[o] = na;
            }
        } else {                                                    // D (H_w + H_{w+3}) -> blocks 0 and 3 of window w
            const int v = u - p.B * T, b = v / W, w = v % W;
            q.gsel[0] = 1;
            q.src[0][0] = frame(b, w); q.src[0][1] = frame(b, w + 3); q.nsrc[0] = 2;
            q.nout = 2;
            for (int o = 0; o < 2; ++o) {
                q.out[o] = blk(b, w, o == 0 ? 0 : 3); q.useacc[o] = 1;
                q.add[o][0] = frame(b, w + 1); q.add[o][1] = frame(b, w + 2); q.nadd[o] = 2;
            }
        }
    } else if (p.mode == WIN_MIX_E2E) {
        const int b = u / (3 * W), w = (u / 3) % W, r = u % 3;
        if (r == 0) {
            q.gsel[0] = 1;
            q.src[0][0] = blk(b, w, 0); q.src[0][1] = blk(b, w, 3); q.nsrc[0] = 2;
            q.nout = 2;
            for (int o = 0; o < 2; ++o) {
                q.out[o] = blk(b, w, o == 0 ? 0 : 3); q.useacc[o] = 1;
                q.add[o][0] = blk(b, w, 1); q.add[o][1] = blk(b, w, 2); q.nadd[o] = 2;
            }
        } else {
            int na = 0;
            q.src[0][0] = blk(b, w, r); q.nsrc[0] = 1;
            q.out[0] = blk(b, w, r); q.useacc[0] = 1; q.nout = 1;
            for (int k2 = 0; k2 < 4; ++k2)
                if (k2 != r) q.add[0][na++] = blk(b, w, k2);
            q.nadd[0] = na;
        }
    } else if (p.mode == WIN_MIX_E2M) {
        const int b = u / W, w = u % W;
        q.src[0][0] = blk(b, w, 1); q.nsrc[0] = 1;
        q.out[0] = mid(b, w); q.useacc[0] = 1; q.nout = 1;
        q.add[0][0] = blk(b, w, 0); q.add[0][1] = blk(b, w, 2); q.add[0][2] = blk(b, w, 3); q.nadd[0] = 3;
    } else if (p.mode == WIN_MIX_M2E) {
        const int b = u / W, w = u % W;
        q.src[0][0] = mid(b, w); q.nsrc[0] = 1;
        q.nout = 4;
        for (int k = 0; k < 4; ++k) {
            q.out[k] = blk(b, w, k); q.useacc[k] = k == 1; q.nadd[k] = k == 1 ? 0 : 1; q.add[k][0] = mid(b, w);
        }
    } else {                                                        // WIN_MIX_E2F
        const int b = u / T, t = u % T;
        q.gsel[1] = 1;
        if (win(t - 1)) q.src[0][q.nsrc[0]++] = blk(b, t - 1, 1);
        if (win(t - 2)) q.src[0][q.nsrc[0]++] = blk(b, t - 2, 2);
        if (win(t)) { q.src[1][q.nsrc[1]++] = blk(b, t, 0); q.src[1][q.nsrc[1]++] = blk(b, t, 3); }
        if (win(t - 3)) { q.src[1][q.nsrc[1]++] = blk(b, t - 3, 0); q.src[1][q.nsrc[1]++] = blk(b, t - 3, 3); }
        int na = 0;
        q.out[0] = frame(b, t); q.useacc[0] = 1; q.nout = 1;
        const int ks[10] = {0, 3, 0, 3, 1, 1, 1, 2, 2, 2}, ss[10] = {1, 1, 2, 2, 0, 2, 3, 0, 1, 3};   // frame t takes block (t - s, k) unmixed
        for (int i = 0; i < 10; ++i)
            if (win(t - ss[i])) q.add[0][na++] = blk(b, t - ss[i], ks[i]);
        q.nadd[0] = na;
    }
}

// a unit's plan by thread 0, then win_mix_body (win_mix_dev.h) runs it: graph 0 = S^, graph 1 = D
__global__ __launch_bounds__(256) void sf_mix_kernel(SfMix p) {
    extern __shared__ __attribute__((aligned(16))) float slab[];            // [Np][NODE_MIX_P]
    __shared__ SfPlan q;
    if (threadIdx.x == 0) sf_plan(p, blockIdx.x, q);
    __syncthreads();
    const float* const graph[2] = {p.S, p.D};
    win_mix_body(q, graph, p.Np, p.N, p.c, p.In, p.Out, slab);            // (F2E: the first and the last frame are in no block 1 or 2: no output)
}

extern "C" int gptst_stfgnn_mix(const float* S, const float* D, int Np, const float* In, float* Out, int c, int mode, int B, int T, int N,
                                void* stream) {
    if (!S || !D || !In || !Out || In == Out || B <= 0 || T < 4 || N <= 0 || mode < 0 || mode > 4) return GPTST_EARG;
    if (Np != 16 * ((N + 15) / 16) || Np > WIN_MIX_MAX_NP || c < 16 || c % 16) return GPTST_ESHAPE;
    const long W = T - 3;
    const long units = mode == WIN_MIX_F2E ? (long)B * (T + W) : mode == WIN_MIX_E2F ? (long)B * T : mode == WIN_MIX_E2E ? (long)B * W * 3 : (long)B * W;
    if (units > 0x7fffffffL) return GPTST_ESHAPE;
    static_assert(WIN_MIX_MAX_NP * NODE_MIX_P * sizeof(float) + sizeof(SfPlan) <= 64 * 1024, "slab + plan exceed the default dynamic LDS");
    const size_t smem = (size_t)Np * NODE_MIX_P * sizeof(float);
    SfMix p{S, D, Np, In, Out, c, mode, B, (int)T, N};
    hipLaunchKernelGGL(sf_mix_kernel, dim3((unsigned)units, (Np / 16 + 3) / 4), dim3(256), smem, (hipStream_t)stream, p);
    GPTST_CHECK_LAUNCH();
    return GPTST_OK;
}
