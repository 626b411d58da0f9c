// bp_relay_device.hip -- Relay-BP with the marginals M_j in a device-memory workspace: the MD = true instantiations of qd_bp_relay_kernel
// (bp_relay_kernel.h), for windows whose LDS form does not fit the CU (QLP [[1020,136]] W = 3: 190 KB with the marginals, 115 KB without)
// and for QD_RELAY_FLAG_MARGINALS_DEVICE.  A file of its own so that each form's instantiations can be listed and bounded by themselves.
#include "bp_relay_kernel.h"

hipError_t qd_launch_bp_relay_device(const BpGraphDev &g, const DecodeArgs &a, const RelayArgs &x, int64_t B, hipStream_t s)
{
    if (!x.marg_ws) return hipErrorInvalidValue;          // (a launch without its workspace would write through a null row)
    return qd_relay_launch_form<true>(g, a, x, B, s);
}
