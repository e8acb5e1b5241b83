// debug_stage.hpp -- the device buffers of one runner call of the test hooks (batch_debug.cpp, equilibrate_debug.cpp);
// test builds only
#pragma once
#ifdef CHIP_TESTING
#include <vector>

#include "host_util.hpp"

namespace chip {

// one buffer per distinct host array (so operands that alias on the host alias on the device), NULL stays NULL; out()
// arrays are uploaded too and copied back by finish()
struct DebugStage {
    DevPool mem;
    struct Buf {
        const void *host;
        void *dev;
        size_t bytes;
        bool out;
    };
    std::vector<Buf> bufs;
    template <typename T> int map(const T *host, size_t len, bool is_out, T **devp) {
        *devp = nullptr;
        if (!host) return CHIP_OK;
        for (Buf &b : bufs)
            if (b.host == (const void *)host) {
                b.out = b.out || is_out;
                *devp = (T *)b.dev;
                return CHIP_OK;
            }
        int rc = mem.upload(devp, host, len);
        if (rc) return rc;
        bufs.push_back(Buf{host, *devp, len * sizeof(T), is_out});
        return CHIP_OK;
    }
    template <typename T> int in(const T *host, size_t len, const T **devp) {
        T *d;
        int rc = map(host, len, false, &d);
        *devp = d;
        return rc;
    }
    template <typename T> int out(T *host, size_t len, T **devp) { return map(host, len, true, devp); }
    int finish(hipStream_t s) {
        CHIP_HIP(hipGetLastError());
        CHIP_HIP(hipStreamSynchronize(s));
        for (const Buf &b : bufs)
            if (b.out && b.bytes) CHIP_HIP(hipMemcpy((void *)b.host, b.dev, b.bytes, hipMemcpyDeviceToHost));
        return CHIP_OK;
    }
};

} // namespace chip
#endif
