// Host side of libprgpu.so, the C-ABI declared in include/prgpu.h: the error string, the version,
// device memory accounting, the context (one HIP stream, HIP events for kernel timing), pr_dev_*.
// The stages are in cns_api.cpp, iter_api.cpp, xchg_api.cpp, mask_api.cpp, lrset_api.cpp,
// sw_api.cpp, seed_api.cpp, siam_api.cpp and bam_api.cpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "ctx.h"

static thread_local std::string g_err;
int set_error(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

extern "C" const char *pr_last_error(void) { return g_err.c_str(); }
extern "C" const char *pr_version(void) { return "prgpu 0.1.0 (gfx950)"; }

// ---------------------------------------------------------------------------
// device memory of the library's buffers (all contexts of the process), and PRGPU_MEM_TRACE=1:
// every growth to stderr with the buffer's group and index (sizing at scale)
std::atomic<int64_t> g_dev_bytes{0};
static bool mem_trace() {
    static const bool on = [] { const char *e = std::getenv("PRGPU_MEM_TRACE"); return e && *e && *e != '0'; }();
    return on;
}
// per-group accounting behind pr_mem_stats (groups are the DevBuf tags and "sw")
namespace {
struct MemGroup {
    char name[16];
    int64_t cur, peak, at_peak;
};
std::mutex g_mem_mu;
MemGroup g_mem[16];
int g_mem_n = 0;
int64_t g_mem_peak = 0;
}   // namespace
void prgpu_mem_note(const char *grp, int id, int64_t delta) {
    const int64_t tot = g_dev_bytes.fetch_add(delta) + delta;
    {
        std::lock_guard<std::mutex> lk(g_mem_mu);
        // "sw CIGAR spill" and the like count under their group's first word
        char key[16] = {};
        for (int i = 0; i < 15 && grp[i] && grp[i] != ' '; ++i) key[i] = grp[i];
        int k = 0;
        while (k < g_mem_n && std::strcmp(g_mem[k].name, key) != 0) ++k;
        if (k == g_mem_n && g_mem_n < 16) {
            std::memcpy(g_mem[k].name, key, 16);
            g_mem[k].cur = g_mem[k].peak = g_mem[k].at_peak = 0;
            ++g_mem_n;
        }
        if (k < g_mem_n) {
            g_mem[k].cur += delta;
            g_mem[k].peak = std::max(g_mem[k].peak, g_mem[k].cur);
        }
        if (tot > g_mem_peak) {
            g_mem_peak = tot;
            for (int j = 0; j < g_mem_n; ++j) g_mem[j].at_peak = g_mem[j].cur;
        }
    }
    if (mem_trace() && delta > 0)
        std::fprintf(stderr, "[prgpu mem] %s[%d] +%.1f MB -> %.2f GB\n", grp, id, delta / 1e6, tot / 1e9);
}

extern "C" int pr_mem_stats(int64_t *cur, int64_t *peak, pr_mem_group *groups, int cap, int *n_groups) {
    std::lock_guard<std::mutex> lk(g_mem_mu);
    if (cur) *cur = g_dev_bytes.load();
    if (peak) *peak = g_mem_peak;
    const int n = std::min(g_mem_n, std::max(cap, 0));
    for (int k = 0; groups && k < n; ++k) {
        std::memcpy(groups[k].name, g_mem[k].name, 16);
        groups[k].cur = g_mem[k].cur;
        groups[k].peak = g_mem[k].peak;
        groups[k].at_total_peak = g_mem[k].at_peak;
    }
    if (n_groups) *n_groups = g_mem_n;
    return 0;
}

extern "C" void pr_mem_reset_peak(void) {
    std::lock_guard<std::mutex> lk(g_mem_mu);
    g_mem_peak = g_dev_bytes.load();
    for (int k = 0; k < g_mem_n; ++k) g_mem[k].peak = g_mem[k].at_peak = g_mem[k].cur;
}
int prgpu_oom(const char *grp, int id, size_t want) {
    size_t fr = 0, total = 0;
    (void)hipMemGetInfo(&fr, &total);
    (void)hipGetLastError();
    return set_error(PR_ERR_HIP, "hipMalloc(%zu) failed (%s[%d]; the library holds %.2f GB, device free %.2f of %.2f GB)",
                     want, grp, id, g_dev_bytes.load() / 1e9, fr / 1e9, total / 1e9);
}

extern "C" int pr_device_count(int *n) {
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess) c = 0;
    *n = c;
    return 0;
}

extern "C" int pr_ctx_create(int device, pr_ctx **out) {
    if (!out) return set_error(PR_ERR_ARG, "null out");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0)
        return set_error(PR_ERR_HIP, "no HIP device visible (libprgpu needs an MI355X)");
    if (device < 0) HIPCHK(hipGetDevice(&device));
    if (device >= n) return set_error(PR_ERR_ARG, "device %d >= count %d", device, n);
    HIPCHK(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return set_error(PR_ERR_HIP, "device %d is %s, libprgpu is built for gfx950", device, prop.gcnArchName);
    pr_ctx *c = new pr_ctx();
    c->device = device;
    auto tag = [](DevBuf *b, int n, const char *g) {
        for (int i = 0; i < n; ++i) b[i].grp = g, b[i].id = i;
    };
    tag(c->cb, CB_COUNT, "cns");
    tag(c->pb, PB_COUNT, "pipe");
    tag(c->mb, MB_COUNT, "mask");
    tag(c->sd, SD_COUNT, "seed");
    tag(c->xb, XB_COUNT, "xchg");
    tag(c->ls, LS_COUNT, "lrset");
    tag(c->eb, EB_COUNT, "bamenc");
    tag(c->sw.buf, SWB_COUNT, "sw");
    c->n_cu = prop.multiProcessorCount;
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
        delete c;
        return set_error(PR_ERR_HIP, "hipStreamCreate failed");
    }
    for (auto &e : c->ev) (void)hipEventCreate(&e);
    *out = c;
    return 0;
}

extern "C" void pr_ctx_destroy(pr_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    for (auto &b : c->cb) b.release();
    for (auto &b : c->pb) b.release();
    for (auto &b : c->mb) b.release();
    for (auto &b : c->sd) b.release();
    for (auto &b : c->xb) b.release();
    for (auto &b : c->ls) b.release();
    for (auto &b : c->eb) b.release();
    sw_release(c->sw);
    for (auto &e : c->ev) (void)hipEventDestroy(e);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

extern "C" int pr_ctx_sync(pr_ctx *c) {
    if (!c) return set_error(PR_ERR_ARG, "null ctx");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int pr_dev_alloc(pr_ctx *c, int64_t bytes, void **dev) {
    if (!c || !dev || bytes < 0) return set_error(PR_ERR_ARG, "bad arg");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMalloc(dev, (size_t)(bytes ? bytes : 16)));
    HIPCHK(hipMemsetAsync(*dev, 0, (size_t)(bytes ? bytes : 16), c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int pr_dev_free(pr_ctx *c, void *dev) {
    if (!c) return set_error(PR_ERR_ARG, "null ctx");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (dev) HIPCHK(hipFree(dev));
    return 0;
}

extern "C" int pr_dev_download(pr_ctx *c, void *host, const void *dev, int64_t bytes) {
    if (!c || bytes < 0 || (bytes && (!host || !dev))) return set_error(PR_ERR_ARG, "bad arg");
    HIPCHK(hipSetDevice(c->device));
    if (bytes) HIPCHK(hipMemcpyAsync(host, dev, (size_t)bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int pr_dev_upload(pr_ctx *c, void *dev, const void *host, int64_t bytes) {
    if (!c || bytes < 0 || (bytes && (!host || !dev))) return set_error(PR_ERR_ARG, "bad arg");
    HIPCHK(hipSetDevice(c->device));
    if (bytes) HIPCHK(hipMemcpyAsync(dev, host, (size_t)bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

int pr_set_error(int code, const char *msg) { return set_error(code, "%s", msg); }
