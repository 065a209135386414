// explicit instantiation: band 15, two jobs per lane, the instances of banded_gotoh_pair_b15_sub.hip with two cells' substitution words
// to an LDS read (PF_SUBLDS | PF_SUBLDS2), which the library launches: the generic fetches and every streamed form, each for
// |G_e| = 0 ... 3.  (NVBIO_HIP_PAIR_SUB = 2 keeps one read per cell, = 1 the v_perm_b32 lookup)
#include "banded_gotoh_pair.h"
namespace nvb {
#define NVB_INST(CELL, F) template hipError_t launch_band_pair<15, CELL, (F)>(const GotohParams&, hipStream_t);
NVB_PAIR_INSTANCES_B15_SUB2(NVB_INST)
#undef NVB_INST
}
