// Move-only owners of what the context (cpf_context.h) gets from the HIP runtime: device and pinned host memory, events, streams.
// A member of one of these types is released when the struct that holds it dies or is assigned over -- the only calls of
// hipFree, hipHostFree, hipEventDestroy and hipStreamDestroy on the context's behalf are the four deleters below.  Every owner
// converts to its raw handle, so kernels' launchers and the runtime take it as they took the pointer.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <utility>

// (hidden: private to the library, and so is every template instantiated over them -- the exported symbols stay the C-ABI's)
#pragma GCC visibility push(hidden)
namespace cpf {

template <typename H, typename Del>
class Owned {
public:
    Owned() = default;
    Owned(const Owned&) = delete;
    Owned& operator=(const Owned&) = delete;
    Owned(Owned&& o) noexcept : h_(std::exchange(o.h_, H{})) {}
    Owned& operator=(Owned&& o) noexcept { if (this != &o) { reset(); h_ = std::exchange(o.h_, H{}); } return *this; }
    ~Owned() { reset(); }
    void reset() { if (h_) { Del{}(h_); h_ = H{}; } }
    void swap(Owned& o) noexcept { std::swap(h_, o.h_); }
    H get() const { return h_; }
    operator H() const { return h_; }
protected:
    H h_{};
};

struct DevFree { void operator()(void* p) const { (void)hipFree(p); } };
struct HostFree { void operator()(void* p) const { (void)hipHostFree(p); } };
struct EventDestroy { void operator()(hipEvent_t e) const { (void)hipEventDestroy(e); } };
struct StreamDestroy { void operator()(hipStream_t s) const { (void)hipStreamDestroy(s); } };

// `count` elements of device memory, never less than 16 bytes: an empty table still has an address (cpf_dev_alloc's rule).
// alloc() frees what the buffer held first; after a failure the buffer is empty.
template <typename T>
struct DevBuf : Owned<T*, DevFree> {
    hipError_t alloc(size_t count) {
        this->reset();
        return hipMalloc((void**)&this->h_, std::max<size_t>(count * sizeof(T), 16));
    }
};
template <typename T>
struct PinnedBuf : Owned<T*, HostFree> {
    hipError_t alloc(size_t count) {
        this->reset();
        return hipHostMalloc((void**)&this->h_, count * sizeof(T), hipHostMallocDefault);
    }
};
struct Event : Owned<hipEvent_t, EventDestroy> {
    hipError_t create(unsigned flags) { reset(); return hipEventCreateWithFlags(&h_, flags); }
};
struct Stream : Owned<hipStream_t, StreamDestroy> {
    hipError_t create(unsigned flags) { reset(); return hipStreamCreateWithFlags(&h_, flags); }
};

}  // namespace cpf
#pragma GCC visibility pop
