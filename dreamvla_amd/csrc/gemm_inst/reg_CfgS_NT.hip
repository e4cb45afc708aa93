#include "../gemm_impl.h"
namespace dvla_gemm { template void launch_one<CfgS, false, true>(const GemmKArgs&, int, hipStream_t); }
