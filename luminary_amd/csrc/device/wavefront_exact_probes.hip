// The truth probes in the exact arithmetic flavour (flavour.h, kernels_probe.h): compiled with the exact flavour's flags (luminary_amd/build.py), apart from the
// render's kernels in wavefront_exact.hip.
#if defined(LUM_FAST) && LUM_FAST
#error "wavefront_exact_probes.hip is part of the exact flavour"
#endif
#include "kernels_probe.h"
