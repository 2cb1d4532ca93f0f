// tests/c/hip_sim/hip/hip_runtime.h -- just enough of the HIP runtime's names for tests/c/surface_kernels_sim.cpp to compile
// grok_amd/csrc/kernels_surface.hip as host C++: a launch becomes loops over blocks and threads, one thread after the other (the two
// surface kernels have no barrier and no cross-lane operation, so that is what they compute).
#pragma once
#include <cstdint>
#include <cstring>
#define __device__
#define __host__
#define __global__
#define __forceinline__ inline
#define __launch_bounds__(...)
struct alignas(8) uint2 { uint32_t x, y; };
struct alignas(16) uint4 { uint32_t x, y, z, w; };
static inline uint4 make_uint4(uint32_t x, uint32_t y, uint32_t z, uint32_t w) { return uint4{x, y, z, w}; }
struct dim3 { uint32_t x, y, z; dim3(uint32_t a = 1, uint32_t b = 1, uint32_t c = 1) : x(a), y(b), z(c) {} };
static dim3 threadIdx, blockIdx;
template <class A, class B> static inline uint64_t min(A a, B b) { return (uint64_t)a < (uint64_t)b ? (uint64_t)a : (uint64_t)b; }
typedef int hipError_t;
typedef struct hip_sim_stream* hipStream_t;
enum { hipSuccess = 0, hipErrorInvalidValue = 1 };
static inline hipError_t hipGetLastError() { return hipSuccess; }
#define hipLaunchKernelGGL(kernel, grid, block, lds, stream, arg) do { const dim3 g_ = grid, b_ = block; \
    for (uint32_t bz_ = 0; bz_ < g_.z; ++bz_) for (uint32_t by_ = 0; by_ < g_.y; ++by_) for (uint32_t bx_ = 0; bx_ < g_.x; ++bx_) \
        for (uint32_t t_ = 0; t_ < b_.x; ++t_) { blockIdx = dim3(bx_, by_, bz_); threadIdx = dim3(t_, 0, 0); kernel(arg); } } while (0)
