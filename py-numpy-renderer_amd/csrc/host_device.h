// host_device.h -- what every host file needs of the device: the error text, the library's stream, growable device
// buffers and the copies to and from them.
#pragma once

namespace {

thread_local std::string g_error;

int fail(int code, const std::string &msg)
{
    g_error = msg;
    return code;
}

#define HIP_TRY(expr)                                                                         \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return fail(MR_E_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_));      \
    } while (0)

hipStream_t g_stream = nullptr;
bool g_initialised = false;

constexpr int MAX_SLOTS = 32;     // frame slots of a scene: the streams it can be rendered from

int ensure_init()
{
    if (g_initialised) return MR_OK;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(MR_E_DEVICE, "no HIP device visible: libmi355rast has no CPU fallback");
    HIP_TRY(hipStreamCreateWithFlags(&g_stream, hipStreamNonBlocking));
    g_initialised = true;
    return MR_OK;
}

// growable device allocation
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    hipError_t ensure(size_t bytes)
    {
        if (bytes <= cap) return hipSuccess;
        if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
        size_t want = bytes + bytes / 4 + 256;
        hipError_t e = hipMalloc(&p, want);
        if (e == hipSuccess) cap = want;
        return e;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    template <class T> T *as() const { return static_cast<T *>(p); }
};

// ensure(), for a buffer whose readers count on zeroes they did not write: when the allocation moved (or the caller
// calls what it holds `stale`), its first `clear_bytes` bytes (0: all of it) are cleared on `stream`
int ensure_cleared(DevBuf &buf, size_t bytes, hipStream_t stream, size_t clear_bytes = 0, bool stale = false)
{
    const void *had = buf.p;
    HIP_TRY(buf.ensure(bytes));
    if (buf.p != had || stale) HIP_TRY(hipMemsetAsync(buf.p, 0, clear_bytes ? clear_bytes : buf.cap, stream));
    return MR_OK;
}

template <class T>
int upload(DevBuf &buf, const std::vector<T> &v, hipStream_t s)
{
    HIP_TRY(buf.ensure(std::max<size_t>(v.size() * sizeof(T), 16)));
    if (!v.empty()) HIP_TRY(hipMemcpyAsync(buf.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, s));
    return MR_OK;
}

template <class T>
int read_back(const DevBuf &buf, T *out, size_t count, const char *what)
{
    if (!out) return fail(MR_E_INVALID, "NULL argument");
    if (!buf.p) return fail(MR_E_INVALID, std::string(what) + ": nothing rendered yet");
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, buf.p, count * sizeof(T), hipMemcpyDeviceToHost));
    return MR_OK;
}

inline unsigned blocks_for(long long n, int per_block) { return (unsigned)std::max<long long>(1, (n + per_block - 1) / per_block); }

}  // namespace
