// dual_halo_sig_kernel<WgSigRpv3, 1, 1> (see dual_halo_sig_body.h)
#include "dual_halo_sig_body.h"

DUAL_SIG_DEFINE(dual_sig_rpv3_tm1, WgSigRpv3, 1)
