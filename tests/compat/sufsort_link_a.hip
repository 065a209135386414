// tests/compat/sufsort_link_a.hip -- one of two translation units that include nvbio/sufsort/sufsort.h and are linked into one library
// (with sufsort_link_b.hip): a header of the drop-in layer must not define anything that two includers cannot share.
#include <nvbio/sufsort/sufsort.h>

extern "C" __attribute__((visibility("default"))) unsigned sufsort_link_a(void) { return sizeof(nvbio::BWTParams); }
