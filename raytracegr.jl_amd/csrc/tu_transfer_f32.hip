// tu_transfer_f32.hip — the Float32 kernels of volume emission (rtgr_transfer.hpp): see tu_transfer_f64.hip.
#include "rtgr_transfer.hpp"
namespace rtgr {
template int transfer_launch<float>(const TransferArgs<float>&, hipStream_t);
template int flow_launch<float>(const FlowArgs<float>&, hipStream_t);
}  // namespace rtgr
