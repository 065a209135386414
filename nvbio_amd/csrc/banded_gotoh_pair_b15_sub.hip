// explicit instantiation: band 15, two jobs per lane, the column frame's cell with the library's row and literals (PF_ROW2 | PF_CONST2)
// and the substitution words read from LDS (PF_SUBLDS), which the library launches: the generic fetches and every streamed form, each
// for |G_e| = 0 ... 3.  (banded_gotoh_pair_b15_lit.hip holds the same instances with the v_perm_b32 lookup, behind NVBIO_HIP_PAIR_SUB = 1)
#include "banded_gotoh_pair.h"
namespace nvb {
#define NVB_INST(CELL, F) template hipError_t launch_band_pair<15, CELL, (F)>(const GotohParams&, hipStream_t);
NVB_PAIR_INSTANCES_B15_SUB(NVB_INST)
#undef NVB_INST
}
