// launch.hpp -- the one way the HIP units launch a kernel (<<<>>>: HIP translation units only).
#pragma once
#include <hip/hip_runtime.h>

#include <utility>

namespace bhmm {

// lets kernel k take more than the default 64 KiB of dynamic LDS (a no-op below that)
template <typename... P>
hipError_t allow_lds(void (*k)(P...), size_t lds)
{
    if (lds <= 64 * 1024)
        return hipSuccess;
    return hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)lds);
}

// launches k<<<grid, block, lds, s>>>(a...) (arguments convert as in a plain call); returns the
// error of the LDS attribute or of the launch
template <typename... P, typename... A>
hipError_t launch(void (*k)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t s, A &&...a)
{
    const hipError_t e = allow_lds(k, lds);
    if (e != hipSuccess)
        return e;
    k<<<grid, block, lds, s>>>(std::forward<A>(a)...);
    return hipGetLastError();
}

} // namespace bhmm
