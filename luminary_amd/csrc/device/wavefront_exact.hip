// The wavefront kernels in the exact arithmetic flavour (flavour.h): this file is compiled with -ffp-contract=off -fno-fast-math (luminary_amd/build.py)
// from the very same headers as the fast flavour in wavefront_fast.hip. The flavour-neutral kernels are not here: kernels_shared.h, compiled in host/core.hip.
#if defined(LUM_FAST) && LUM_FAST
#error "wavefront_exact.hip is the exact flavour: build it without -DLUM_FAST=1"
#endif
#include "wavefront_table_impl.h"
