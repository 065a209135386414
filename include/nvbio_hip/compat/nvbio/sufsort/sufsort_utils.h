// compat/nvbio/sufsort/sufsort_utils.h -- the reference keeps SetBWTHandler here (nvbio/sufsort/sufsort_utils.h:57-81); in the drop-in
// layer it lives with the functions that call it.
#pragma once
#include "sufsort.h"
