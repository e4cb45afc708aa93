// measurement build of the phase kernel (gemm_phase.h PHASE_STAMPS; gemm.hip variant 89): NN layout, plain epilogue, s_memtime
// stamps for tests/probes/gemm_probe.cpp --stamps.  Compiled only with -DDVLA_GEMM_STAMPS (DVLA_ABLATIONS=1 builds).
#ifdef DVLA_GEMM_STAMPS
#include "../gemm_phase.h"
namespace dvla_gemm { template void launch_phase_one<false, false, 0, PHASE_STAMPS>(const GemmKArgs&, int, hipStream_t); }
#endif
