// The slab product sg_nodemix_kernel (stgcn.hip), st_step_kernel (stgode.hip) and win_mix_body (win_mix_dev.h: ss_mix_kernel of stsgcn.hip and
// sf_mix_kernel of stfgnn.hip) share: a wave's 16-node tile of L (rows n0 .. n0 + 15 of an (Np, Np) matrix read from L2) times the 32-channel
// slab of a unit's Np rows in LDS, added into two 16 x 16 accumulators (channels j, j + 16).  Filling the slab and the epilogue are the callers'
// own: the two window mixes have theirs in common, in win_mix_body; the other two differ from it and from each other.  ag_attmix_kernel (astgcn.hip: per-sample masked tiles of L, a 64-channel slab,
// the next tile of L prefetched into registers) is a different loop and stays apart; so does the recurrences' 64-column loop (tgcn.hip, msdr.hip: a slab
// at pitch 68, a wave owning one column tile for NT row tiles, L prefetched one step ahead): recur_step_dev.h's recur_mix_tiles.
#pragma once
#include "common.h"

#define NODE_MIX_P 36       // pitch of the slab, in floats: 32 channels + 4

// lp = L + (n0 + j) Np + 4 kk: this lane's row of the tile, at its k offset
__device__ __forceinline__ void node_mix_slab(f32x4 (&acc)[2], const float* lp, const float* slab, int Np, int j, int kk) {
    for (int m0 = 0; m0 < Np; m0 += 16) {
        const float4 a = ld4(lp + m0);
        const float av[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float* sp = slab + (m0 + 4 * kk + e) * NODE_MIX_P + j;
            acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[e], sp[0], acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[e], sp[16], acc[1], 0, 0, 0);
        }
    }
}
