// Instantiations of the SGNS kernels for VEC = 2 (d in (64, 128]).
#include "come_sgns_impl.h"

COME_DEFINE_VEC(2)
