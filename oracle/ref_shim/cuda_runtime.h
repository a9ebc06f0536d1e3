// Stand-in for <cuda_runtime.h>, on the include path only while oracle/ref_kernels.py compiles the reference's three
// kernel files for gfx950.  It holds a name mapping and nothing else: the runtime names those files use, spelled in HIP.
// The wave-wide shuffle mask of __shfl_down_sync is dropped: every lane of a wave takes part in the reference's reductions.
#pragma once
#define HIP_DISABLE_WARP_SYNC_BUILTINS 1
#include <hip/hip_runtime.h>

#define cudaError_t hipError_t
#define cudaSuccess hipSuccess
#define cudaGetLastError hipGetLastError
#define cudaGetErrorString hipGetErrorString
#define cudaDeviceSynchronize hipDeviceSynchronize
#define cudaMemset hipMemset
#define __shfl_down_sync(mask, value, offset) __shfl_down(value, offset)
