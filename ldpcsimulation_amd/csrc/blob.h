// blob.h -- a host image of several arrays that go to the device as one allocation
// and one copy (host_rt.h upload): the graph and the schedules of a context. Every
// section starts at a multiple of `align`; the kernels get base + the offset add()
// returned. No HIP: the host sanitizer build (tests/native/host_asan.cpp) checks the
// offsets against the layouts the contexts have always used.
#pragma once
#include <cstddef>
#include <cstring>
#include <vector>

namespace ldpc {

class Blob {
public:
    explicit Blob(size_t align) : align_(align) {}
    // Appends `bytes` bytes of src and returns their offset. The section takes
    // max(bytes, room) bytes rounded up to the alignment, the rest zero: an empty
    // section takes nothing, and the next one starts where it would have.
    size_t add(const void *src, size_t bytes, size_t room = 0)
    {
        const size_t at = buf_.size(), n = bytes > room ? bytes : room;
        buf_.resize(at + (n + align_ - 1) / align_ * align_, 0);
        if (bytes) std::memcpy(buf_.data() + at, src, bytes);
        return at;
    }
    template <class T> size_t add(const std::vector<T> &v) { return add(v.data(), sizeof(T) * v.size()); }
    const unsigned char *data() const { return buf_.data(); }
    size_t size() const { return buf_.size(); }

private:
    size_t align_;
    std::vector<unsigned char> buf_;
};

}  // namespace ldpc
