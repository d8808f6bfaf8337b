// hsw_gadget_call.hpp -- what the calls of the proving round over caller-owned device columns share
// (hsw_gadget_permuted.cpp, _product.cpp, _permutation.cpp, _ntt.cpp, _msm.cpp, _open.cpp, _shplonk.cpp, _quotient.cpp):
// the refusals, the overlap sweep, the gadget's scratch, its staging, the stage events and the end of a call.
// Internal: not part of the boundary.
#ifndef HSW_GADGET_CALL_HPP
#define HSW_GADGET_CALL_HPP

#include <string>

#include "hsw_gadget_launch.hpp"

namespace hsw {

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// "<kind> <i>: <what>" as the engine's error, with `status`
inline int fail_at(hsw_engine *e, int status, const char *kind, size_t i, const char *what) {
    return hsw_engine_fail(e, status, (std::string(kind) + " " + std::to_string(i) + ": " + what).c_str());
}

// the representation of the pass for a call that takes 32-byte cells: HSW_OK and *montgomery, or the refusal
inline int pass_cells(const Context &c, bool *montgomery) {
    uint32_t repr = 0;
    if (pass_repr(c, &repr) != HSW_OK) return hsw_engine_fail(c.engine, HSW_ERR_UNSUPPORTED, "the batches of the pass differ in representation");
    if ((repr | c.repr_flags) & HSW_REPR_COMPACT64) return hsw_engine_fail(c.engine, HSW_ERR_UNSUPPORTED, "32-byte cells only");
    *montgomery = (repr & HSW_REPR_MONTGOMERY) != 0;
    return HSW_OK;
}

// 32 stored bytes as a field element; false: not below p
inline bool load_below_p(PFe &x, const void *stored) {
    std::memcpy(&x, stored, 32);
    return pfe_below_p(x);
}

// bytes [lo, hi) that item `index` of a call writes (out) or reads; other: whatever else the caller wants to name
struct Interval { uintptr_t lo, hi; size_t index; bool out; size_t other; };
// An output may overlap neither another output nor anything read: one sweep in address order, with the furthest end of
// the outputs (and whose it is) and of all intervals seen so far.  true: *writer is the output at fault and *with the
// interval it overlaps (sorts iv)
inline bool output_overlaps(std::vector<Interval> &iv, Interval *writer, Interval *with) {
    std::sort(iv.begin(), iv.end(), [](const Interval &x, const Interval &y) { return x.lo < y.lo; });
    uintptr_t end_out = 0, end_any = 0;
    Interval last_out{}, last_any{};
    for (const Interval &x : iv) {
        if (x.out ? x.lo < end_any : x.lo < end_out) {
            *writer = x.out ? x : last_out;
            *with = x.out ? last_any : x;
            return true;
        }
        if (x.out && x.hi > end_out) { end_out = x.hi; last_out = x; }
        if (x.hi > end_any) { end_any = x.hi; last_any = x; }
    }
    return false;
}

// DeviceScratch (hsw_gadget.hpp): the one block of device memory the calls of the round stage into and work in
// (hsw_gadget::scratch).  A call that needs more frees the block and only then allocates exactly what it needs, so the
// peak is the new block alone; a failure leaves the scratch empty.  Safe because every call that uses the scratch has
// synchronised its stream before it returns: nothing on the device still reads the old block, and no call leaves
// anything in it that a later one reads.  Both inside an EngineScope
inline void DeviceScratch::release() { (void)hipFree(d); d = nullptr; cap = 0; }
inline int DeviceScratch::reserve(size_t bytes) {
    if (bytes <= cap) return HSW_OK;
    release();
    const hipError_t he = hipMalloc(&d, bytes);
    if (he != hipSuccess) { d = nullptr; return hip_status(he); }
    cap = bytes;
    return HSW_OK;
}

// base + offset as a T *: the sections of a Staging on the device, or in its host image
template <class T>
T *at(void *base, size_t offset) { return reinterpret_cast<T *>(static_cast<uint8_t *>(base) + offset); }

// The layout of a call in the scratch, every section 256-aligned: first what is uploaded (`host`, its image, zeroed
// unless filled; the status words come first), then what only the launches write (work).  Each returns its offset
struct Staging {
    std::vector<uint8_t> host;
    size_t bytes = 0;                               // of the whole layout: what the call reserves
    size_t zeroed(size_t n) {                       // (an empty section still gets a slot)
        const size_t o = host.size();
        host.resize(align256(o + std::max<size_t>(n, 1)), 0);
        bytes = host.size();
        return o;
    }
    size_t add(const void *src, size_t n) {
        const size_t o = zeroed(n);
        if (src && n) std::memcpy(host.data() + o, src, n);
        return o;
    }
    size_t work(size_t n) {                         // (after the last uploaded section; the end is not padded)
        const size_t o = align256(bytes);
        bytes = o + n;
        return o;
    }
    template <class T>
    T *image(size_t offset) { return at<T>(host.data(), offset); }
};

struct Events {                                     // the stage boundaries of one call
    std::vector<hipEvent_t> ev;
    ~Events() { for (hipEvent_t e : ev) (void)hipEventDestroy(e); }
    hipError_t record(hipStream_t s) {
        hipEvent_t e = nullptr;
        hipError_t he = hipEventCreate(&e);
        if (he != hipSuccess) return he;
        ev.push_back(e);
        return hipEventRecord(e, s);
    }
};

// the start of a call's device work: the image uploaded to the scratch, then the first event
inline hipError_t upload(const Staging &st, void *d, hipStream_t stream, Events &ev) {
    const hipError_t he = hipMemcpyAsync(d, st.host.data(), st.host.size(), hipMemcpyHostToDevice, stream);
    return he == hipSuccess ? ev.record(stream) : he;
}

// The end of it, `he` being how the launches went: the first `bytes` of the scratch copied to `back`, the stream waited
// for, ms[i] the time between events i and i + 1.  HSW_OK, or the HIP error as the engine's
inline int finish(hsw_engine *e, hipError_t he, hipStream_t stream, const Events &ev, const void *d, void *back, size_t bytes,
                  std::vector<float> &ms) {
    if (he == hipSuccess) he = hipMemcpyAsync(back, d, bytes, hipMemcpyDeviceToHost, stream);
    if (he == hipSuccess) he = hipStreamSynchronize(stream);
    ms.assign(ev.ev.empty() ? 0 : ev.ev.size() - 1, 0.0f);
    for (size_t i = 0; he == hipSuccess && i < ms.size(); i++) he = hipEventElapsedTime(&ms[i], ev.ev[i], ev.ev[i + 1]);
    e->timed = false;
    return he == hipSuccess ? HSW_OK : hsw_engine_fail(e, HSW_ERR_HIP, hipGetErrorString(he));
}

}  // namespace hsw
#endif
