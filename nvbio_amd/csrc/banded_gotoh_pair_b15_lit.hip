// explicit instantiation: band 15, two jobs per lane, the column frame's cell with the row and the constants' placement the library
// launches for it (PF_ROW2 | PF_CONST2): the generic fetches and every streamed form, each for |G_e| = 0 ... 3
#include "banded_gotoh_pair.h"
namespace nvb {
#define NVB_INST(CELL, F) template hipError_t launch_band_pair<15, CELL, (F)>(const GotohParams&, hipStream_t);
NVB_PAIR_INSTANCES_B15_LIT(NVB_INST)
#undef NVB_INST
}
