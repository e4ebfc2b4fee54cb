// The integer hash behind every deterministic stream of the library (kernels_synth.hip, kernels_restage.hip) and their numpy
// twins (cellector_amd/synth.py, restage.py): the splitmix64 finaliser and its golden-ratio increment.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#define GOLD 0x9E3779B97F4A7C15ull

__host__ __device__ __forceinline__ uint64_t mix64(uint64_t z)
{
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}
