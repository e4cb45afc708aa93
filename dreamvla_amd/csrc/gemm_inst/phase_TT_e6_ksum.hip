// the phase kernel's fp32 class WITH the k-sum code (gemm_phase.h PHASE_KSUM): TT layout = the weight gradients that also
// produce a bias gradient; the second = the same with a partial last K-tile (PHASE_TAIL)
#include "../gemm_phase.h"
namespace dvla_gemm {
template void launch_phase_one<true, true, 6, PHASE_KSUM>(const GemmKArgs&, int, hipStream_t);
template void launch_phase_one<true, true, 6, PHASE_TAIL | PHASE_KSUM>(const GemmKArgs&, int, hipStream_t);
}
