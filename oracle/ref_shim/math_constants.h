/* Stand-in for the CUDA toolkit's <math_constants.h>: the three constants the reference's kernels name,
 * with the values the toolkit documents (pi rounded to binary32, +inf, a quiet NaN). */
#pragma once
#include <limits>
#define CUDART_PI_F 3.141592654f
#define CUDART_INF_F (std::numeric_limits<float>::infinity())
#define CUDART_NAN_F (std::numeric_limits<float>::quiet_NaN())
