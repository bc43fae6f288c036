// What the host code of the engine (engine.h) and of the training path (train_impl.h) both stand on: the exception that carries a
// GL_ERR_* code, printf-style message formatting, and the bump allocator every activation lives in (defined in engine.hip).
#pragma once
#include <cstdarg>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

#include "common.h"

namespace gl {

struct GlError : std::runtime_error {
    int code;
    GlError(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

inline std::string fmt(const char* f, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, f);
    vsnprintf(buf, sizeof(buf), f, ap);
    va_end(ap);
    return buf;
}

// Bump allocator over one hipMalloc'd slab with stack-style scopes. Addresses are a pure
// function of the allocation sequence, so a captured hipGraph replays against the same buffers.
class Arena {
   public:
    void init(size_t bytes);
    void destroy();
    void* alloc(size_t bytes);
    template <class T> T* get(size_t n) { return reinterpret_cast<T*>(alloc(n * sizeof(T))); }
    size_t mark() const { return off_; }
    void release(size_t m) { off_ = m; }
    void reset() { off_ = 0; }
    size_t capacity() const { return cap_; }
    size_t high_water() const { return hw_; }
    size_t committed() const { return vmm_ ? mapped_ : cap_; }   // device memory actually behind the reservation

   private:
    void grow(size_t need);
    char* base_ = nullptr;
    size_t cap_ = 0, off_ = 0, hw_ = 0;
    // virtual-memory form: `cap_` bytes of ADDRESSES are reserved (the bump sequence, and with it every address a captured graph
    // holds, is a pure function of the allocation sequence), physical memory is mapped behind them in chunks as the high-water
    // mark rises -- a context costs what it uses, not what it was told it might
    bool vmm_ = false;
    size_t mapped_ = 0, gran_ = 0;
    std::vector<void*> handles_;   // hipMemGenericAllocationHandle_t, one per mapped chunk
    int dev_ = 0;
};

}  // namespace gl
