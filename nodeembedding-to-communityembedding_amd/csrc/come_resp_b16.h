// come_resp_b16.h -- the bf16-part images of the upper precision factors (gfx950): the block table
// and LDS layout (RespB16) and the kernel that packs them (k_pack_upper_b16), shared by the E-step
// (k_gmm_resp_b16, come_gmm_estep.hip, which describes the layout) and the community loss
// (k_comm_loss_b16, come_community_loss.hip).
#pragma once

#include "come_c4.h"

namespace come {

template <int D>
struct RespB16 {
    static constexpr int NS = D / 32, CT = D / 16;
    static constexpr int NB = CT == 8 ? 20 : 6;     // sum over ct of ct / 2 + 1
    static constexpr int BLK = 3 * 1024;
    static constexpr int NW = 8, NU = 2;
    static constexpr int UB = NB / NU, UBYTES = UB * BLK;
    static constexpr int PAR = 2 * UBYTES, PARF = 256 + 64;
    static constexpr int LDS_BYTES = PAR + 2 * PARF * 4;
    static constexpr int PIECES = UBYTES / 1024;
    int ct[NB], s[NB];
    constexpr RespB16() : ct(), s() {
        int n = 0;
        for (int c = 0; c < CT; ++c)
            for (int k = 0; k <= c / 2; ++k) {
                ct[n] = c;
                s[n] = k;
                ++n;
            }
    }
    __host__ __device__ static constexpr int at(int P, int i, int g) {
        return P * 1024 + i * 64 + 16 * (g ^ (((i >> 2) & 1) << 1));
    }
};

template <int D>
__global__ void __launch_bounds__(256) k_pack_upper_b16(const float *__restrict__ P,
                                                        char *__restrict__ img, int K) {
    using R = RespB16<D>;
    constexpr R TB{};
    const int64_t n = (int64_t)K * R::NB * 16 * 4;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < n;
         t += (int64_t)gridDim.x * 256) {
        const int g = (int)(t & 3), i = (int)((t >> 2) & 15);
        const int64_t kb = t >> 6;  // k * NB + block
        const int b = (int)(kb % R::NB);
        const int64_t k = kb / R::NB;
        const int c = 16 * TB.ct[b] + i, f0 = 32 * TB.s[b] + 8 * g;
        const float *Pk = P + k * D * D;
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = Pk[(int64_t)(f0 + e) * D + c];  // P^T[c][f] = P[f][c]
        uint4 w[3];
        uint32_t *w1 = &w[0].x, *w2 = &w[1].x, *w3 = &w[2].x;
#pragma unroll
        for (int e = 0; e < 4; ++e) bf16_split3(v[2 * e], v[2 * e + 1], w1[e], w2[e], w3[e]);
        char *blk = img + kb * R::BLK;
#pragma unroll
        for (int p = 0; p < 3; ++p) *reinterpret_cast<uint4 *>(blk + R::at(p, i, g)) = w[p];
    }
}

}  // namespace come
