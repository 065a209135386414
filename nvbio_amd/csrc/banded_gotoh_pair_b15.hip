// explicit instantiation: band 15, two jobs per lane, the three cells; the generic fetches and every streamed form; the column frame's
// cell also with the row the library launches for it (PF_ROW2)
#include "banded_gotoh_pair.h"
namespace nvb {
#define NVB_INST(F) \
    template hipError_t launch_band_pair<15, P16, (F)>(const GotohParams&, hipStream_t); \
    template hipError_t launch_band_pair<15, PM3, (F)>(const GotohParams&, hipStream_t); \
    template hipError_t launch_band_pair<15, PD3, (F)>(const GotohParams&, hipStream_t); \
    template hipError_t launch_band_pair<15, PD3, (F) | PF_ROW2>(const GotohParams&, hipStream_t);
NVB_INST(PF_SINK_VCC) NVB_PAIR_STREAM_FORMS(NVB_INST)
#undef NVB_INST
}
