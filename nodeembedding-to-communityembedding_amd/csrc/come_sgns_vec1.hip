// Instantiations of the SGNS kernels for VEC = 1 (d in (0, 64]).
#include "come_sgns_impl.h"

COME_DEFINE_VEC(1)
