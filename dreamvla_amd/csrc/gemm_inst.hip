// gemm_inst.hip -- one GEMM launcher instantiation (and with it its kernel) per compilation.  gemm_inst_list.h names every
// instance once; the build compiles this file once per entry of that list, with -DDVLA_INST=<the entry's text>, so that every
// instance is a translation unit of its own and the build runs in parallel.  gemm.hip reads the same list as `extern template`.
#ifndef DVLA_INST
#error "compile with -DDVLA_INST=<one entry of gemm_inst_list.h>, e.g. -DDVLA_INST='DVLA_EXTERN_RING(RCfgL, true, false, 4)'"
#endif
#include "gemm_phase.h"

namespace dvla_gemm {
#define DVLA_EXTERN_REG(CF, AT, BT) template void launch_one<CF, AT, BT>(const GemmKArgs&, int, hipStream_t);
#define DVLA_EXTERN_RING(RC, AT, BT, EPI) template void launch_ring_one<RC, AT, BT, EPI>(const GemmKArgs&, int, hipStream_t);
#define DVLA_EXTERN_PHASE(AT, BT, EPI, FEAT) template void launch_phase_one<AT, BT, EPI, FEAT>(const GemmKArgs&, int, hipStream_t);
DVLA_INST
}  // namespace dvla_gemm
