// HD: a function of a header that kernels and plain C++ share -- __host__ __device__ under hipcc, inline under g++ (the CPU tests under tests/cpp compile such
// headers without a GPU).
#pragma once
#if defined(__HIPCC__)
#define HD __host__ __device__ inline
#else
#define HD inline
#endif
