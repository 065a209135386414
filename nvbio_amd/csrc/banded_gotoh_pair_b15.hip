// explicit instantiation: band 15, two jobs per lane, both cells
#include "banded_gotoh_pair.h"
namespace nvb {
template hipError_t launch_band_pair<15, P16>(const GotohParams&, hipStream_t);
template hipError_t launch_band_pair<15, PM3>(const GotohParams&, hipStream_t);
}
