// The window mix ss_mix_kernel (stsgcn.hip) and sf_mix_kernel (stfgnn.hip) share: a workgroup's unit is a plan, and this is what runs it.
// A plan is up to NPH phases, each the product of one of two (Np, Np) graphs with a slab that is the sum of up to NSRC source blocks of the
// input, all phases added into the same accumulators; then up to NOUT output blocks, each the accumulator (or nothing) plus up to NADD blocks
// of the input unmixed.  Blocks are named by their first row (of N) in In / Out.  Which blocks a unit of each of the five forms below takes is
// the predictors' own: ss_plan (windows of three frames, one graph, one phase) and sf_plan (four frames, two graphs, two phases for E2F) stay
// in their units and fill this struct; thread 0 writes it into LDS, a barrier, then every thread calls win_mix_body.
// The order of every sum is fixed: sources in plan order, phases in order, the accumulator and then the adds in plan order.
// The slab product itself is node_mix_slab (node_mix_dev.h), which sg_nodemix_kernel (stgcn.hip) and st_step_kernel (stgode.hip) run under a
// fill and an epilogue of their own.
#pragma once
#include "common.h"
#include "node_mix_dev.h"

#define WIN_MIX_MAX_NP 448  // 448 * NODE_MIX_P * 4 = 64 512 bytes of slab + a plan: under the 64 KB of dynamic LDS a launch gets by default

// the five forms of a mix, by the row layouts (frames, expanded, middle) of its input and output
#define WIN_MIX_F2E 0
#define WIN_MIX_E2E 1
#define WIN_MIX_E2M 2
#define WIN_MIX_M2E 3
#define WIN_MIX_E2F 4

// phase h: acc += graph[gsel[h]] (sum of its nsrc[h] source blocks); output o = [useacc[o]] acc + the sum of its nadd[o] blocks of In
template <int NPH, int NSRC, int NOUT, int NADD>
struct WinMixPlan {
    static constexpr int phases = NPH;
    int nout;
    int gsel[NPH], nsrc[NPH];
    long src[NPH][NSRC];
    long out[NOUT];
    int useacc[NOUT], nadd[NOUT];
    long add[NOUT][NADD];
};

// one unit and four 16-node tiles per workgroup of 256; 32 channels of the unit's source rows in LDS at a time (slab [Np][NODE_MIX_P]), the
// graphs read from L2.  q is in LDS and complete (the caller's barrier).  The phase loop stays rolled: unrolled, the two-phase instantiation
// doubles its MFMA and grows by a tenth for nothing.  With one phase the graph select and the empty-phase skip fold away.
template <class Plan>
__device__ __forceinline__ void win_mix_body(const Plan& q, const float* const (&graph)[2], int Np, int N, int c, const float* In, float* Out,
                                             float* slab) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, kk = lane >> 4;
    const int n0 = (blockIdx.y * 4 + wave) * 16;
    const bool active = n0 < Np;
    const int nout = q.nout;
    if (nout == 0) return;                                                  // (the same for every thread of the workgroup)
    for (int cg = 0; cg * 32 < c; ++cg) {
        f32x4 acc[2];
        acc[0] = acc[1] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
        for (int h = 0; h < Plan::phases; ++h) {
            const int nsrc = q.nsrc[h];
            if (Plan::phases > 1 && nsrc == 0) continue;                    // (the same for every thread of the workgroup)
            __syncthreads();                                                // the previous product's reads of the slab are done
            for (int f = tid; f < Np * 8; f += 256) {
                const int m = f >> 3, c4 = f & 7;
                float4 v = f4zero();
                if (m < N && 32 * cg + 4 * c4 < c) {
                    for (int s = 0; s < nsrc; ++s) {
                        const float4 a = ld4(In + (size_t)(q.src[h][s] + m) * c + 32 * cg + 4 * c4);
                        v.x += a.x; v.y += a.y; v.z += a.z; v.w += a.w;
                    }
                }
                st4(slab + m * NODE_MIX_P + 4 * c4, v);
            }
            __syncthreads();
            if (active) node_mix_slab(acc, (Plan::phases > 1 && q.gsel[h] ? graph[1] : graph[0]) + (size_t)(n0 + j) * Np + 4 * kk, slab, Np, j, kk);
        }
        if (!active) continue;
        // ---- epilogue in the accumulator layout: reg r = (node n0 + kk*4 + r, channel 32 cg + 16 ct + j) ----
        for (int o = 0; o < nout; ++o) {
            const long ob = q.out[o];
            const int useacc = q.useacc[o], na = q.nadd[o];
#pragma unroll
            for (int ct = 0; ct < 2; ++ct) {
                const int ch = 32 * cg + 16 * ct + j;
                if (ch >= c) continue;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int n = n0 + kk * 4 + r;
                    if (n >= N) continue;
                    float v = useacc ? acc[ct][r] : 0.f;
                    for (int a = 0; a < na; ++a) v += In[(size_t)(q.add[o][a] + n) * c + ch];
                    Out[(size_t)(ob + n) * c + ch] = v;
                }
            }
        }
    }
}
