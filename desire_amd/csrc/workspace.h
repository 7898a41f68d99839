// workspace.h -- the one owner of a handle's named device buffers (desire_ctx::ws, the workspace, and desire_ctx::dev, the packed weights).
// Host code only, no ROCm header: the allocator is two function pointers that ctx.h binds to hipMalloc / hipFree and
// tests/c_host/workspace_driver.cpp to a counting fake.  The rules:
//   - ensure() is the only way a buffer comes to exist.  An entry always holds a live allocation: a failed allocation leaves the name as if it
//     had never been requested, so the next call tries again instead of finding a name without memory behind it.
//   - reads (find / get / bytes) never insert and never throw: an unknown name is nullptr / 0.  No exception leaves through the C ABI.
//   - a buffer that is held and large enough is never moved, so pointers handed to kernels or captured in a hipGraph stay valid.
#pragma once
#include <cstddef>
#include <map>
#include <string>

struct DevBuf {
    void* p = nullptr; size_t bytes = 0;                     // bytes: as requested (a request of 0 bytes holds a 4-byte allocation)
    float* f() const { return static_cast<float*>(p); }
};

struct WsItem { const char* n; size_t bytes; };              // one entry of an allocation list

struct Workspace {
    typedef int (*AllocFn)(void** p, size_t bytes);          // 0: *p holds `bytes` bytes of device memory
    typedef void (*FreeFn)(void* p);
    Workspace(AllocFn a, FreeFn f) : alloc_(a), free_(f) {}
    Workspace(const Workspace&) = delete;
    Workspace& operator=(const Workspace&) = delete;

    const DevBuf* find(const char* name) const { const auto it = m_.find(name); return it == m_.end() ? nullptr : &it->second; }
    template <class T = float> T* get(const char* name) const { const DevBuf* b = find(name); return b ? static_cast<T*>(b->p) : nullptr; }
    size_t bytes(const char* name) const { const DevBuf* b = find(name); return b ? b->bytes : 0; }
    size_t size() const { return m_.size(); }

    // `name` holds at least `bytes` bytes afterwards (0), or does not exist (non-zero: the allocation failed).  Held and large enough: nothing
    // happens.  Otherwise the old buffer is freed and a new one allocated; *fresh tells the caller that the contents are new (uninitialised).
    int ensure(const char* name, size_t bytes, bool* fresh = nullptr) {
        if (fresh) *fresh = false;
        const auto it = m_.find(name);
        if (it != m_.end()) {
            if (it->second.bytes >= bytes) return 0;
            free_(it->second.p);
            m_.erase(it);
        }
        void* p = nullptr;
        if (alloc_(&p, bytes ? bytes : 4) || !p) return -1;
        m_[name] = DevBuf{p, bytes};
        if (fresh) *fresh = true;
        return 0;
    }
    // every buffer of a list, in order; stops at the first failure and names it (the ones before it stay held, the next call allocates the rest)
    int ensure_all(const WsItem* list, size_t n, std::string* failed) {
        for (size_t i = 0; i < n; ++i)
            if (ensure(list[i].n, list[i].bytes)) { if (failed) *failed = list[i].n; return -1; }
        return 0;
    }
    void release(const char* name) { const auto it = m_.find(name); if (it != m_.end()) { free_(it->second.p); m_.erase(it); } }
    void release_all() { for (auto& kv : m_) free_(kv.second.p); m_.clear(); }

private:
    AllocFn alloc_; FreeFn free_;
    std::map<std::string, DevBuf, std::less<>> m_;           // (transparent compare: a lookup by const char* builds no std::string)
};
