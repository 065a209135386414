// tests/compat/sufsort_link_b.hip -- the second includer of nvbio/sufsort/sufsort.h; see sufsort_link_a.hip.
#include <nvbio/sufsort/sufsort.h>
#include <nvbio/sufsort/sufsort_utils.h>

extern "C" __attribute__((visibility("default"))) unsigned sufsort_link_b(void) { return sizeof(nvbio::SetBWTHandler); }
