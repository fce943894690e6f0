// dual_halo_sig_kernel<WgSigMnist2, 1, 1> (see dual_halo_sig_body.h)
#include "dual_halo_sig_body.h"

DUAL_SIG_DEFINE(dual_sig_mnist2_tm1, WgSigMnist2, 1)
