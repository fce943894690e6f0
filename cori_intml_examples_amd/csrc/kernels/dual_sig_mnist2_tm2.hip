// dual_halo_sig_kernel<WgSigMnist2, 1, 2> (see dual_halo_sig_body.h)
#include "dual_halo_sig_body.h"

DUAL_SIG_DEFINE(dual_sig_mnist2_tm2, WgSigMnist2, 2)
