// What the forward row GEMMs with their weight rows in LDS share: sg_tapgemm_kernel (stgcn.hip) and ss_wingemm_kernel (stsgcn.hip),
//   Y[row][ch] = epi(sum over k of Xs[row][k] W[ch][k] + bias[ch])
// A workgroup of ROW_GEMM_THREADS owns a column block of 16 NCT weight rows, all K of them in LDS at pitch K + 4, the biases behind them; a wave
// owns 16-row tiles and the NCT column tiles of 16.  GLU: the first NCT / 2 column tiles are P channels, the other half the Q channels (weight
// rows co + ch) of the same outputs, so a lane holds P and Q of one (row, channel) pair.
//   row_gemm_stage   stages the weight rows and biases of column block blockIdx.y (rows past the last channel: zero); it alone knows the map
//                    from a row of the block to its channel and weight row.  Returns the block's first channel.
//   row_gemm_plan    host side: the launch plan both launches derive, and the tiles-per-wave queries of the tests with them
//   glu_bwd_store    the GLU's other half: the store of its derivative in the two gate_bwd kernels
// The loop over a wave's tiles and the epilogue stay in the two kernels: one walker over row and epilogue policies was built and measured, and
// cost ss_wingemm_kernel occupancy and 3 - 9 % of its launches' time (profiles/downstream_rowgemm_ab.txt).
// mt_tapgemm_kernel (mtgnn.hip) shares nothing here: it walks K in 128-wide chunks through static LDS with TPW row tiles per wave and skips
// a tap no row of the workgroup has (__syncthreads_or); a staging function serving both would branch on its caller in every line.
#pragma once
#include "common.h"

#define ROW_GEMM_THREADS 512

template <int NCT>
__device__ __forceinline__ int row_gemm_stage(float* smem, const float* Wg, const float* bg, int Ktot, int co, bool glu) {
    constexpr int OCW = 16 * NCT, half = OCW / 2;
    const int P = Ktot + 4, tid = threadIdx.x;
    float* Wl = smem;                       // [OCW][P]
    float* bl = Wl + OCW * P;               // [OCW]
    const int c0 = blockIdx.y * (glu ? half : OCW);
    // row l of the block: its channel, and the weight (and bias) row that holds it
    auto wrow = [&](int l, int& ch) {
        ch = glu ? (l < half ? c0 + l : c0 + l - half) : c0 + l;
        return glu && l >= half ? co + ch : ch;
    };
    const int k4 = Ktot >> 2;
    for (int f = tid; f < OCW * k4; f += ROW_GEMM_THREADS) {
        const int l = f / k4, c4 = f - l * k4;
        int ch;
        const int wr = wrow(l, ch);
        st4(Wl + l * P + 4 * c4, ch < co ? ld4(Wg + (size_t)wr * Ktot + 4 * c4) : f4zero());
    }
    if (tid < OCW) {
        int ch;
        const int wr = wrow(tid, ch);
        bl[tid] = (bg != nullptr && ch < co) ? bg[wr] : 0.f;
    }
    __syncthreads();
    return c0;
}

// the GLU's derivative (out = A S, S = sigma(Q)): [g S | g A S (1 - S)] for four channels; d = the P half of the row of dPre (2 co = 8 co4 floats)
__device__ __forceinline__ void glu_bwd_store(float* d, int co4, float4 g, float4 s, float4 a) {
    st4(d, make_float4(g.x * s.x, g.y * s.y, g.z * s.z, g.w * s.w));
    st4(d + 4 * co4, make_float4(g.x * a.x * (s.x * (1.f - s.x)), g.y * a.y * (s.y * (1.f - s.y)), g.z * a.z * (s.z * (1.f - s.z)),
                                 g.w * a.w * (s.w * (1.f - s.w))));
}

// ---- the launch plan: the one place that derives it, for the launches and for the queries of the tests ----
// ntiles row tiles and co output channels in column blocks of ocw = 64 (wide) or 32 weight rows (GLU: ocw / 2 outputs), `groups` times over in gridDim.z (the
// windows of STSGCN): as many row blocks as give about `target` workgroups, each wave then working through tpw tiles
struct RowGemmPlan { bool wide; int ocw, colblocks, rowblocks, tpw; };

static inline RowGemmPlan row_gemm_plan(long ntiles, int co, bool glu, bool wide, long groups, int target) {
    RowGemmPlan g;
    g.wide = wide; g.ocw = wide ? 64 : 32;
    const int per = glu ? g.ocw / 2 : g.ocw, wpb = ROW_GEMM_THREADS / 64;
    g.colblocks = (co + per - 1) / per;
    long rowblocks = target / (g.colblocks * groups); if (rowblocks < 1) rowblocks = 1;
    long tpw = (ntiles + wpb * rowblocks - 1) / (wpb * rowblocks); if (tpw < 1) tpw = 1;
    g.tpw = (int)tpw;
    g.rowblocks = (int)((ntiles + wpb * tpw - 1) / (wpb * tpw));
    return g;
}
