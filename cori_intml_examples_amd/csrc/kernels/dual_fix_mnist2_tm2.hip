// dual_halo_fix_kernel<DgSigMnist2, 2> (see dual_halo_fix_body.h)
#include "dual_halo_fix_body.h"

DUAL_FIX_DEFINE(dual_fix_mnist2_tm2, DgSigMnist2, 2)
