#include "../gemm_impl.h"
namespace dvla_gemm { template void launch_one<CfgS, true, true>(const GemmKArgs&, int, hipStream_t); }
