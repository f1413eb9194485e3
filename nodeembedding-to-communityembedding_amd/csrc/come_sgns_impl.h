// come_sgns_impl.h -- the SGNS trainer kernels (come_sgns_common.h: what they share and the
// execution model; come_sgns_o2.h; come_sgns_o1.h) and the table of their instantiations.
#pragma once
#include "come_sgns_common.h"
#include "come_sgns_o2.h"
#include "come_sgns_o1.h"

namespace come {

// Kernel entry addresses per instantiation (defined in come_sgns_vec{1,2,4,8}.hip so the
// instantiations compile in parallel).
struct KernelSet {
    void *o2_direct[2][3];  // [FULL][maxn idx]
    void *o2_ring[2][3];    // sequential mode
    void *o2_stream[2][3];  // Hogwild mode
    void *o2_stream_win[2];  // Hogwild mode with quiet rows: VEC <= 2, n <= 5 (else nullptr)
    void *o1[2][3];
    void *o1_runs[2][3];
};

// The code object lists its kernels in the order they are named here.
template <int VEC, bool FULL, int MAXN>
void add_kernels(KernelSet &k, int mi) {
    k.o2_direct[FULL][mi] = (void *)&k_sgns_o2<VEC, FULL, MAXN>;
    k.o1[FULL][mi] = (void *)&k_sgns_o1<VEC, FULL, MAXN>;
    k.o1_runs[FULL][mi] = (void *)&k_sgns_o1_runs<VEC, FULL, MAXN>;
    k.o2_ring[FULL][mi] = (void *)&k_sgns_o2_ring<VEC, FULL, MAXN>;
    k.o2_stream[FULL][mi] = (void *)&k_sgns_o2_stream<VEC, FULL, MAXN>;
}

template <int VEC, bool FULL>
void add_window_kernel(KernelSet &k) {
    k.o2_stream_win[FULL] = (void *)&k_sgns_o2_stream<VEC, FULL, 5, true>;
}

// Every kernel of one row width.  FULL (d == 64 VEC: no bounds test per element) exists from
// VEC = 2 on, d = 64 runs the bounded VEC = 1 kernels; the windowed stream kernel exists at
// VEC <= 2, n <= 5.
template <int VEC>
KernelSet make_kernel_set() {
    KernelSet k{};
    add_kernels<VEC, false, 5>(k, 0);
    add_kernels<VEC, false, 10>(k, 1);
    add_kernels<VEC, false, 20>(k, 2);
    if constexpr (VEC > 1) {
        add_kernels<VEC, true, 5>(k, 0);
        add_kernels<VEC, true, 10>(k, 1);
        add_kernels<VEC, true, 20>(k, 2);
    }
    if constexpr (VEC <= 2) add_window_kernel<VEC, false>(k);
    if constexpr (VEC == 2) add_window_kernel<VEC, true>(k);
    return k;
}

#define COME_DECLARE_VEC(V) \
    const KernelSet &kernels_vec##V(); \
    hipError_t upload_exp_table_vec##V(const float *host1000);
COME_DECLARE_VEC(1)
COME_DECLARE_VEC(2)
COME_DECLARE_VEC(4)
COME_DECLARE_VEC(8)
#undef COME_DECLARE_VEC

}  // namespace come

// The whole of come_sgns_vecV.hip: the kernels of width V, and the upload of that code object's
// copy of c_exp_table.
#define COME_DEFINE_VEC(V)                                                  \
    namespace come {                                                        \
    const KernelSet &kernels_vec##V() {                                     \
        static const KernelSet ks = make_kernel_set<V>();                   \
        return ks;                                                          \
    }                                                                       \
    hipError_t upload_exp_table_vec##V(const float *host1000) {             \
        return hipMemcpyToSymbol(HIP_SYMBOL(c_exp_table), host1000,         \
                                 sizeof(float) * kExpTableSize);            \
    }                                                                       \
    }
