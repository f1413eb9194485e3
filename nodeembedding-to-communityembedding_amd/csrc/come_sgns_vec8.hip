// Instantiations of the SGNS kernels for VEC = 8 (d in (256, 512]).
#include "come_sgns_impl.h"

COME_DEFINE_VEC(8)
