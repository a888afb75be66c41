// Stand-in for <c10/cuda/CUDAGuard.h>.  The reference names
// at::cuda::OptionalCUDAGuard only inside a macro that its host entry points
// expand; those entry points are not part of the host build (oracle/ref.py), so
// nothing is needed here.
#pragma once
