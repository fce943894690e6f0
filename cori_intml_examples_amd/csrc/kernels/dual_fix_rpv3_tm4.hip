// dual_halo_fix_kernel<DgSigRpv3, 4> (see dual_halo_fix_body.h)
#include "dual_halo_fix_body.h"

DUAL_FIX_DEFINE(dual_fix_rpv3_tm4, DgSigRpv3, 4)
