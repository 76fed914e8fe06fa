// What the two recurrences share: tg_step_kernel (tgcn.hip) and ms_step_kernel (msdr.hip).  A workgroup of RECUR_THREADS owns NT 16-node row tiles
// of one sample and runs
//   mix    M = L[tile rows, :] In_b     In_b 64 columns at a time in an LDS slab [Np][RECUR_SP]; wave w owns column tile w of the 64
//   GEMM   P = A Wt^T                   A rows in LDS at a pitch, Wt (NO, K) row-major from L2; wave w owns column tiles w, w + 4, ...
// both with fp32 MFMA 16x16x4 in the accumulator layout reg r = (row 4 kk + r, column j), j = lane & 15, kk = lane >> 4.
//   recur_mix_tiles    the L x slab product of one wave for its NT row tiles, the next 16 columns of L fetched one step ahead of their use
//   recur_gemm_tiles   one output column tile of the GEMM for NT row tiles, four k-blocks of weight loads in flight
//   recur_tiles, recur_check, recur_launch    host side: the rows-per-workgroup rule, the argument and shape conditions both families test, and
//                      the launch with the dynamic-LDS attribute above 64 KB (per device, per kernel instantiation, once per size)
// Only inner loops and the launch are here, and nothing branches on its caller.  Filling the slab (TGCN's mode-specific loads, its bwd cand forming
// dpre1 on load; MSDR's identity block behind it), where M and P go, every epilogue, the LDS size functions and the C entries stay in the two
// units: the loop around a fill is four lines, and one walker over loaders and epilogues is what cost ss_wingemm_kernel 3 - 9 % (row_gemm_dev.h,
// DESIGN.md section 21).
// recur_mix_tiles serves ms_step_kernel only.  tg_step_kernel keeps the same loop written out: called through the function (same source, same
// MFMA count, VGPRs equal or 4 lower) its launches timed alone came out above the spread of the kernel with its own copy — one row tile per
// workgroup: fwd gates 55.5 -> 56.1 us, fwd state 45.4 -> 45.7, bwd state 67.5 -> 68.4; two, in a second call: bwd state 47.0 -> 47.2.  A build
// with only that loop written out again measured equal in every line, one with only the GEMM loop written out did not.  Everything else
// measured equal to the copies it replaces (profiles/recurrence_step_ab.txt).
#pragma once
#include "common.h"

#define RECUR_THREADS 256
#define RECUR_SP 68                  // pitch of the 64-column operand slab: 4 kk-rows apart = 272 floats = 16 banks apart, conflict-free ds_read_b32
#define RECUR_MAX_DEVICES 64
#define RECUR_LDS_MAX (160 * 1024)

// acc[nt] = L[n0 + 16 nt .. + 15, :] slab[:, 16 wave .. + 15];  tv[nt]: row tile nt lies inside the Np padded rows (else its rows of L are not read)
template <int NT>
__device__ __forceinline__ void recur_mix_tiles(f32x4 (&acc)[NT], const float* L, int Np, int n0, const bool (&tv)[NT], const float* slab, int wave,
                                                int j, int kk) {
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float4 an[NT];                                             // the graph rows come from L2: fetched one step ahead of their use
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) an[nt] = tv[nt] ? ld4(L + (size_t)(n0 + 16 * nt + j) * Np + 4 * kk) : f4zero();
    for (int m0 = 0; m0 < Np; m0 += 16) {
        float4 a[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            a[nt] = an[nt];
            if (tv[nt] && m0 + 16 < Np) an[nt] = ld4(L + (size_t)(n0 + 16 * nt + j) * Np + m0 + 16 + 4 * kk);
        }
        const float* sp = slab + (m0 + 4 * kk) * RECUR_SP + 16 * wave + j;
        const float bv[4] = {sp[0], sp[RECUR_SP], sp[2 * RECUR_SP], sp[3 * RECUR_SP]};
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[nt].x, bv[0], acc[nt], 0, 0, 0);
            acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[nt].y, bv[1], acc[nt], 0, 0, 0);
            acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[nt].z, bv[2], acc[nt], 0, 0, 0);
            acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[nt].w, bv[3], acc[nt], 0, 0, 0);
        }
    }
}

// acc[nt] = Al[16 nt .. + 15, :K] Wt[16 ct .. + 15, :K]^T;  Al in LDS at `pitch` floats a row, K a multiple of 16
template <int NT>
__device__ __forceinline__ void recur_gemm_tiles(f32x4 (&acc)[NT], const float* Al, int pitch, const float* Wt, int K, int ct, int j, int kk) {
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const float* wp = Wt + (size_t)(16 * ct + j) * K + 4 * kk;
    const float* mp = Al + j * pitch + 4 * kk;
    for (int q0 = 0; q0 < K; q0 += 64) {                       // the weights come from L2: four k-blocks of loads in flight at a time
        float4 w[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) w[i] = q0 + 16 * i < K ? ld4(wp + q0 + 16 * i) : f4zero();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (q0 + 16 * i >= K) break;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const float4 a = ld4(mp + 16 * nt * pitch + q0 + 16 * i);
                acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, w[i].x, acc[nt], 0, 0, 0);
                acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, w[i].y, acc[nt], 0, 0, 0);
                acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, w[i].z, acc[nt], 0, 0, 0);
                acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, w[i].w, acc[nt], 0, 0, 0);
            }
        }
    }
}

// ---- host side ----
// row tiles per workgroup: 2 while that still leaves more workgroups than the chip has CUs, else 1 (a small batch must not collapse the grid)
static inline int recur_tiles(int B, int Np, int forced) {
    if (forced == 1 || forced == 2) return forced;
    const int tiles = Np / 16;
    return (long)B * ((tiles + 1) / 2) > 256 ? 2 : 1;
}

// the conditions every step launch tests: arguments first, then shapes
static inline int recur_check(const float* Wt, int B, int T, int N, int t, int tiles, int Hp, int Np) {
    if (!Wt || B <= 0 || B > 65535 || T <= 0 || N <= 0 || t < 0 || t >= T || tiles < 0 || tiles > 2) return GPTST_EARG;
    if (Hp < 16 || Hp > 128 || Hp % 16 || Np != 16 * ((N + 15) / 16)) return GPTST_ESHAPE;
    return GPTST_OK;
}

template <auto KERNEL, class P>
static int recur_launch(const P& p, dim3 grid, size_t smem, hipStream_t stream) {
    if (smem > 64 * 1024) {                    // more than 64 KB of dynamic LDS needs the attribute, on every device this process launches on
        static size_t have[RECUR_MAX_DEVICES] = {};              // (one table per KERNEL)
        int dev = -1;
        if (hipGetDevice(&dev) != hipSuccess || dev < 0) return GPTST_EARG;
        if (dev >= RECUR_MAX_DEVICES || have[dev] < smem) {
            const hipError_t e = hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
            if (e != hipSuccess) return (int)e;
            if (dev < RECUR_MAX_DEVICES) have[dev] = smem;       // (a race sets it twice: harmless)
        }
    }
    hipLaunchKernelGGL(KERNEL, grid, dim3(RECUR_THREADS), smem, stream, p);
    GPTST_CHECK_LAUNCH();
    return GPTST_OK;
}
