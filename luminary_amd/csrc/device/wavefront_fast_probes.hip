// The truth probes in the fast arithmetic flavour (flavour.h, kernels_probe.h): compiled with the fast flavour's flags (luminary_amd/build.py), apart from the
// render's kernels in wavefront_fast.hip.
#if !defined(LUM_FAST) || !LUM_FAST
#error "wavefront_fast_probes.hip is the fast flavour: build it with -DLUM_FAST=1"
#endif
#include "kernels_probe.h"
