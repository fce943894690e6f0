// dual_halo_fix_kernel<DgSigRpv2, 4> (see dual_halo_fix_body.h)
#include "dual_halo_fix_body.h"

DUAL_FIX_DEFINE(dual_fix_rpv2_tm4, DgSigRpv2, 4)
