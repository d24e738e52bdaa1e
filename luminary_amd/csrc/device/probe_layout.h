// The word counts of the truth probes' records (kernels_probe.h states what each word holds), defined once: the probe kernels index by them, the host layer
// (csrc/host/probes.hip) sizes its buffers by them and holds them against the LUMC_*_PROBE_* values of include/lum_core.h. Constants only, no device code.
#pragma once

#include <stdint.h>

namespace lum {
// k_light_sample_probe: per vertex (in; the bounce and sun probes read the same vertex) and per thread (out); kLightProbeLanes is dev_light.h's kLightTreeOutputs
constexpr uint32_t kLightProbeVertexWords = 20, kLightProbeLaneWords = 17, kLightProbeHeadWords = 18, kLightProbeLanes = 8;
constexpr uint32_t kLightProbeWords = kLightProbeHeadWords + kLightProbeLanes * kLightProbeLaneWords;
constexpr uint32_t kBounceProbeHeadWords = 44, kBounceProbeTechWords = 24, kBounceProbeLightDirWords = 27;  // k_bounce_probe, per thread (out)
constexpr uint32_t kBounceProbeWordsPerThread = kBounceProbeHeadWords + 3 * kBounceProbeTechWords + kBounceProbeLightDirWords;
constexpr uint32_t kSkyProbeRayWords = 12, kSkyProbeHeadWords = 40, kSkyProbeStepWords = 49, kSkyProbeMaxSteps = 12;  // k_sky_probe, per ray (in) and per thread (out)
constexpr uint32_t kSkyProbeWordsPerThread = kSkyProbeHeadWords + kSkyProbeMaxSteps * kSkyProbeStepWords;
constexpr uint32_t kSunProbeWordsPerThread = 64;  // k_sun_probe, per thread (out)
}  // namespace lum
