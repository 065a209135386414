// explicit instantiation: band 15, two jobs per lane, the three cells; the generic fetches and every streamed form; the column frame's
// cell also with the row the library launches for it (PF_ROW2)
#include "banded_gotoh_pair.h"
namespace nvb {
#define NVB_INST(CELL, F) template hipError_t launch_band_pair<15, CELL, (F)>(const GotohParams&, hipStream_t);
NVB_PAIR_INSTANCES_B15(NVB_INST)
#undef NVB_INST
}
