// bp_relay.hip -- Relay-BP with a shot's whole state in LDS: the MD = false instantiations of qd_bp_relay_kernel (bp_relay_kernel.h), and the
// LDS layout of both forms.  The form whose marginals live in device memory is instantiated in bp_relay_device.hip.
#include "bp_relay_kernel.h"

hipError_t qd_launch_bp_relay(const BpGraphDev &g, const DecodeArgs &a, const RelayArgs &x, int64_t B, hipStream_t s)
{
    return qd_relay_launch_form<false>(g, a, x, B, s);
}

// LDS of the relay kernel over the gather kernel's layout: marginals (LDS form only: marg_device leaves them out, off_marg = -1), best
// candidate, the 64-bit weight sum
int qd_relay_layout(const BpGraphDev &g, bool marg_device, RelayArgs *x)
{
    int off = (g.lds_bytes + 15) & ~15;
    x->off_marg = -1;
    if (!marg_device) { x->off_marg = off; off += ((g.n_pad + 1) * 4 + 15) & ~15; }
    x->off_best = off; off += (g.out_words * 4 + 15) & ~15;
    x->off_wsum = off; off += 16;
    x->lds_bytes = off;
    return off;
}
