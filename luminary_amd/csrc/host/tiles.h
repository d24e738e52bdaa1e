// Host arithmetic of tiles.cpp that has no place in the C ABI.
#pragma once

#include <cstdint>
#include <vector>

__attribute__((visibility("hidden"))) std::vector<uint32_t> undersampling_pixels(uint32_t width, uint32_t height, uint32_t stage, uint32_t iteration);
