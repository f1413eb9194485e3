// Instantiations of the SGNS kernels for VEC = 4 (d in (128, 256]).
#include "come_sgns_impl.h"

COME_DEFINE_VEC(4)
