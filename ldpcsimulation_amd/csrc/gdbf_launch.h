// gdbf_launch.h -- the host-side launch tails the GDBF kernel families (gdbf.hip, rgdbf.hip,
// rstat.hip) share: the template dispatch of a launch and the persistent ticket grid of
// their register-schedule kernels.
#pragma once
#include "gdbf.h"

#include <hip/hip_runtime.h>
#include <type_traits>

namespace ldpc {

// fn(F{}, integral_constant<int, SRC>{}) for the precision and the sample source of a launch.
template <typename Fn>
static hipError_t gdbf_dispatch(bool f64, int src, Fn &&fn)
{
    using Given = std::integral_constant<int, SRC_GIVEN>;
    using Philox = std::integral_constant<int, SRC_PHILOX>;
    if (f64) return src == SRC_GIVEN ? fn(double{}, Given{}) : fn(double{}, Philox{});
    return src == SRC_GIVEN ? fn(float{}, Given{}) : fn(float{}, Philox{});
}

// fn(integral_constant<int, DVM>{}, integral_constant<int, NT>{}) for the register-schedule
// instance a choice names: DVM 4 | 12, NT 512 | 1024.
template <typename Fn>
static hipError_t gdbf_rows_dispatch(const GdbfChoice &ch, Fn &&fn)
{
    using D4 = std::integral_constant<int, 4>;
    using D12 = std::integral_constant<int, 12>;
    using T512 = std::integral_constant<int, 512>;
    using T1024 = std::integral_constant<int, 1024>;
    if (ch.dvm == 4) return ch.threads == 512 ? fn(D4{}, T512{}) : fn(D4{}, T1024{});
    return ch.threads == 512 ? fn(D12{}, T512{}) : fn(D12{}, T1024{});
}

// The persistent grid of a register-schedule kernel: as many workgroups as fit on the device
// (one per CU where the occupancy query fails), no more than there are items; items past the
// first grid's are handed out by *ticket, zeroed here (tickets = false: the kernel strides).
template <typename... KArgs, typename... Args>
static hipError_t gdbf_rows_grid_launch(void (*fn)(KArgs...), int threads, int lds_bytes, unsigned *ticket,
                                        bool tickets, int items, int num_cus, hipStream_t s, Args... args)
{
    if (tickets) {
        if (!ticket) return hipErrorInvalidValue;
        const hipError_t e = hipMemsetAsync(ticket, 0, sizeof(unsigned), s);
        if (e != hipSuccess) return e;
    }
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, threads, lds_bytes) != hipSuccess || per_cu < 1)
        per_cu = 1;
    int grid = per_cu * (num_cus > 0 ? num_cus : 1);
    if (grid > items) grid = items;
    hipLaunchKernelGGL(fn, dim3(grid), dim3(threads), lds_bytes, s, args...);
    return hipGetLastError();
}

}  // namespace ldpc
