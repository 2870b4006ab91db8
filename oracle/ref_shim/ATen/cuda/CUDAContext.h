/* Stand-in for <ATen/cuda/CUDAContext.h>: the host build has one "stream", the calling thread. */
#pragma once
namespace at { namespace cuda {
struct CUDAStream {};
inline CUDAStream getCurrentCUDAStream() { return CUDAStream{}; }
}}
