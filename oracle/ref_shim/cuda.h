// Stand-in for <cuda.h> (the driver API, of which the reference's device code
// uses nothing): see cuda_runtime.h in this directory.
#pragma once
#include "cuda_runtime.h"
