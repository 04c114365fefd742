// devbuf.h -- the two small types the host layer allocates through.
//   Carver : one list of sub-array word counts that is both the size of a staging block and its layout
//            (plain C++, no HIP: FHE_AMD_CARVER_ONLY leaves the rest of this header out)
//   DevBuf : an owned device allocation, freed by its destructor
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <initializer_list>
#include <stdexcept>
#include <string>
#include <vector>

namespace fhe_amd {

// A host entry point first lists its sub-arrays (u64 word counts, in order), reserves words() words, binds the
// block and then takes the sub-arrays in the listed order.  take() checks each request against the list: a request
// out of order, of another size or past the end throws, so size and layout cannot disagree.
class Carver {
public:
    Carver() = default;
    Carver(std::initializer_list<size_t> parts) {
        for (size_t w : parts) add(w);
    }
    void add(size_t words) {
        parts_.push_back(words);
        total_ += words;
    }
    size_t words() const { return total_; }
    void bind(uint64_t* base) {
        base_ = base;
        next_ = 0;
        off_ = 0;
    }
    uint64_t* take(size_t words) {
        if (next_ >= parts_.size()) throw std::logic_error("Carver: more sub-arrays taken than listed");
        if (parts_[next_] != words)
            throw std::logic_error("Carver: sub-array " + std::to_string(next_) + " listed with " +
                                   std::to_string(parts_[next_]) + " words, taken with " + std::to_string(words));
        uint64_t* p = base_ + off_;
        off_ += words;
        ++next_;
        return p;
    }

private:
    std::vector<size_t> parts_;
    size_t total_ = 0, next_ = 0, off_ = 0;
    uint64_t* base_ = nullptr;
};

}  // namespace fhe_amd

#ifndef FHE_AMD_CARVER_ONLY
#include <hip/hip_runtime.h>

namespace fhe_amd {

struct HipError : std::runtime_error {
    hipError_t code;
    HipError(hipError_t e, const std::string& what)
        : std::runtime_error(what + ": " + hipGetErrorString(e)), code(e) {}
};
#define FHE_HIP_CHECK(expr)                                   \
    do {                                                      \
        hipError_t _e = (expr);                               \
        if (_e != hipSuccess) throw HipError(_e, #expr);      \
    } while (0)

// The owners live in a namespace of their own (Engine names them through member aliases): keygen_dev.hip keeps a
// file-local DevBuf<T> for its temporaries.
namespace devmem {

// Move-only owner of one hipMalloc block.  alloc() replaces the block (the old one is freed first, as a key
// reload did by hand); whoever calls it has made sure nothing on the device still reads the old block
// (Engine::reserve for the grow-only scratch).
class DevBuf {
public:
    DevBuf() = default;
    ~DevBuf() { release(); }
    DevBuf(DevBuf&& o) noexcept : p_(o.p_), bytes_(o.bytes_), device_(o.device_) { o.p_ = nullptr; o.bytes_ = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            release();
            p_ = o.p_; bytes_ = o.bytes_; device_ = o.device_;
            o.p_ = nullptr; o.bytes_ = 0;
        }
        return *this;
    }
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;

    void alloc(int device, size_t bytes) {
        release();
        device_ = device;
        FHE_HIP_CHECK(hipSetDevice(device));
        FHE_HIP_CHECK(hipMalloc(&p_, bytes));
        bytes_ = bytes;
    }
    void release() noexcept {
        if (!p_) return;
        (void)hipSetDevice(device_);
        (void)hipFree(p_);
        p_ = nullptr;
        bytes_ = 0;
    }
    template <typename T = void>
    T* as() const { return static_cast<T*>(p_); }
    size_t bytes() const { return bytes_; }

private:
    void* p_ = nullptr;
    size_t bytes_ = 0;
    int device_ = 0;
};

// a DevBuf of T words that reads as a T* where a launcher takes one (null while nothing is allocated)
template <typename T>
struct DevArr : DevBuf {
    operator T*() const { return as<T>(); }
};

}  // namespace devmem
}  // namespace fhe_amd
#endif  // FHE_AMD_CARVER_ONLY
