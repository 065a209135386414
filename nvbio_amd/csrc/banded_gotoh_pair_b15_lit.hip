// explicit instantiation: band 15, two jobs per lane, the column frame's cell with the row and the constants' placement the library
// launches for it (PF_ROW2 | PF_CONST2): the generic fetches and every streamed form, each for |G_e| = 0 ... 3
#include "banded_gotoh_pair.h"
namespace nvb {
#define NVB_INST(F) template hipError_t launch_band_pair<15, PD3, (F)>(const GotohParams&, hipStream_t);
#define NVB_INST_GE(F) NVB_PAIR_GE_FORMS(NVB_INST, F)
NVB_INST_GE(PF_SINK_VCC) NVB_PAIR_STREAM_FORMS(NVB_INST_GE)
#undef NVB_INST_GE
#undef NVB_INST
}
