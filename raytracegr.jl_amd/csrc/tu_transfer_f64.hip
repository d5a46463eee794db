// tu_transfer_f64.hip — the Float64 kernels of volume emission (rtgr_transfer.hpp): transfer_kernel for the five closed right-hand
// sides, the pointwise hook's kernel, and the launch that picks the instantiation a scene's (metric, a) selects.
#include "rtgr_transfer.hpp"
namespace rtgr {
template int transfer_launch<double>(const TransferArgs<double>&, hipStream_t);
template int flow_launch<double>(const FlowArgs<double>&, hipStream_t);
}  // namespace rtgr
