// Weight gradient of a tap GEMM, the body sg_wgrad_kernel (stgcn.hip), mt_wgrad_kernel (mtgnn.hip) and ss_winwgrad_kernel (stsgcn.hip) share
// (the forward's counterpart, for the two of them whose weight rows sit whole in LDS, is row_gemm_dev.h):
//   part[z][o][k] = sum over the rows of split z of D[row][o] Xs[row][k],   bpart[z][o] = column sums of D   (bpart may be NULL)
// Xs[row][k] is X at the row's source row for the tap of column k.  Which row that is — and whether it exists, and a mask on it — is the
// caller's: `src(row, rv)` returns this thread's float4 of Xs[row] (columns kcol .. kcol + 3 with kcol = blockIdx.x * 64 + 4 * (tid % 16)),
// zeros where the row (rv = row < rows), the column or the tap's time step is outside.
// Grid (ceil(Ktot / 64), ceil(cw / 64), splits), 256 threads; split z owns the 64-row chunks [z cps, min(nchunks, (z + 1) cps)).
// A caller whose rows of D are not one contiguous run (ss_winwgrad_kernel, stsgcn.hip: the rows of one window of a (b, w, ...) tensor) passes a
// row map as well: `rmap.split()` is the split whose chunks this workgroup owns, `rmap.slot()` the partial it writes, `rmap(row)` the row of D.
#pragma once
#include "common.h"

#define TAP_WG_P 80         // pitch of the 64 x 64 LDS tiles: 80 mod 64 = 16, so the four k-rows of an operand read land on disjoint banks

// all rows, in order: split blockIdx.z owns its chunks and its partial, row r of D is r
struct TapWgAllRows {
    __device__ __forceinline__ int split() const { return blockIdx.z; }
    __device__ __forceinline__ int slot() const { return blockIdx.z; }
    __device__ __forceinline__ size_t operator()(int row) const { return (size_t)row; }
};

template <class Src, class Rows>
__device__ __forceinline__ void tap_wgrad_body(const float* D, int cw, int Ktot, float* part, float* bpart, int rows, int cps, int nchunks,
                                               const Src& src, const Rows& rmap) {
    __shared__ __attribute__((aligned(16))) float Dl[64 * TAP_WG_P];
    __shared__ __attribute__((aligned(16))) float Xl[64 * TAP_WG_P];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, kk = lane >> 4;
    const int kb = blockIdx.x, cb = blockIdx.y, z = rmap.split(), slot = rmap.slot();
    const int ch0 = z * cps, ch1 = min(nchunks, ch0 + cps);
    // this thread's four float4 of either tile: row rl = i*16 + tid/16, columns 4 (tid % 16)
    const int c4 = tid & 15, rb = tid >> 4;
    const int dcol = cb * 64 + 4 * c4;
    const bool dv = dcol < cw;
    f32x4 acc[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) acc[nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float bsum = 0.f;
    float4 dr[4], xr[4];
    auto fetch = [&](int chunk) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = chunk * 64 + i * 16 + rb;
            const bool rv = row < rows;
            dr[i] = (rv && dv) ? ld4(D + rmap(row) * cw + dcol) : f4zero();
            xr[i] = src(row, rv);
        }
    };
    if (ch0 < ch1) fetch(ch0);
    for (int chunk = ch0; chunk < ch1; ++chunk) {
        __syncthreads();                                   // the previous chunk's reads of the tiles are done
#pragma unroll
        for (int i = 0; i < 4; ++i) { st4(Dl + (i * 16 + rb) * TAP_WG_P + 4 * c4, dr[i]); st4(Xl + (i * 16 + rb) * TAP_WG_P + 4 * c4, xr[i]); }
        __syncthreads();
        if (chunk + 1 < ch1) fetch(chunk + 1);
        if (bpart != nullptr && kb == 0 && tid < 64) {
            for (int rl = 0; rl < 64; ++rl) bsum += Dl[rl * TAP_WG_P + tid];
        }
#pragma unroll 4
        for (int s = 0; s < 16; ++s) {
            const float a = Dl[(4 * s + kk) * TAP_WG_P + 16 * wave + j];
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, Xl[(4 * s + kk) * TAP_WG_P + 16 * nt + j], acc[nt], 0, 0, 0);
        }
    }
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        const int k = kb * 64 + 16 * nt + j;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int o = cb * 64 + 16 * wave + kk * 4 + r;
            if (o < cw && k < Ktot) part[((size_t)slot * cw + o) * Ktot + k] = acc[nt][r];
        }
    }
    if (bpart != nullptr && kb == 0 && tid < 64 && cb * 64 + tid < cw) bpart[(size_t)slot * cw + cb * 64 + tid] = bsum;
}

template <class Src>
__device__ __forceinline__ void tap_wgrad_body(const float* D, int cw, int Ktot, float* part, float* bpart, int rows, int cps, int nchunks,
                                               const Src& src) {
    tap_wgrad_body(D, cw, Ktot, part, bpart, rows, cps, nchunks, src, TapWgAllRows());
}

// The split rule of the partial-writing gradients (the *_nsplit entries of stgcn.hip, stsgcn.hip and mtgnn.hip): `items` (64-row chunks, or
// units) over as many splits as bring the launch's `tiles` output tiles to about 1024 workgroups, at most one split per item; then the
// splits that the resulting items per split leave non-empty.
static inline int wgrad_split_rule(int tiles, int items) {
    int ns = 1024 / tiles; if (ns < 1) ns = 1; if (ns > items) ns = items;
    const int per = (items + ns - 1) / ns;
    return (items + per - 1) / per;
}
