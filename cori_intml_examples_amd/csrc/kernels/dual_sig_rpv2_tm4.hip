// dual_halo_sig_kernel<WgSigRpv2, 1, 4> (see dual_halo_sig_body.h)
#include "dual_halo_sig_body.h"

DUAL_SIG_DEFINE(dual_sig_rpv2_tm4, WgSigRpv2, 4)
