// explicit instantiation: band 15, two jobs per lane
#include "banded_gotoh_pair.h"
namespace nvb { template hipError_t launch_band_pair<15>(const GotohParams&, hipStream_t); }
