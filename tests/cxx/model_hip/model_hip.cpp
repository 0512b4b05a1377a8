// A model of the HIP runtime for host-only builds of the library: the entry points the library leaves undefined, written
// from HIP's documented semantics.  "Device" memory is zero-filled host memory; a stream is an in-order list of ops
// (copy, 2-D copy, memset, event record, wait for event, kernel launch); a kernel does nothing unless the harness gave its
// name a behaviour.  Ops run eagerly, lazily (only when a synchronising call forces them) or on a worker per stream
// (model_hip.h).  Every violated rule becomes a line of the error list.
//
// What is modelled, and where it is documented (HIP Runtime API reference, "Stream management", "Event management",
// "Memory management"):
//  - hipStreamWaitEvent waits for the event's most recent hipEventRecord AT THE TIME OF THE CALL; an event that has never
//    been recorded is complete, and the wait is a no-op;
//  - a blocking hipMemcpy / hipMemset runs on the null stream, which synchronises with blocking streams only: a stream made
//    with hipStreamNonBlocking is not waited for;
//  - hipEventSynchronize / hipStreamSynchronize wait for exactly the record / the stream they name (and, through the
//    stream's own waits, for the records those are bound to);
//  - hipFree and hipHostFree synchronise the device first;
//  - hipHostRegister pins whole pages, and a page cannot be pinned twice.
//
// In the threaded schedule a worker never releases anything a host thread acquires except an op's `done` flag, and host
// threads read that flag with acquire order only inside the synchronising calls (relaxed everywhere else): a dependency
// the library forgot is a data race for ThreadSanitizer, not an ordering the model's own locks happen to supply.
#include "model_hip.h"

#include <hip/hip_runtime_api.h>

#include <atomic>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <set>
#include <string>
#include <thread>
#include <vector>

namespace {

enum OpKind { OP_NOP, OP_COPY, OP_MEMSET, OP_RECORD, OP_WAIT, OP_KERNEL };

struct StreamM;
struct EventM;
struct Hook {
    std::string part;
    std::vector<size_t> arg_bytes;
    model_hip_kernel_run run;
    model_hip_kernel_writes writes;
    void* user;
};

struct Op {
    OpKind kind = OP_NOP;
    StreamM* stream = nullptr;
    std::atomic<Op*> next{nullptr};
    std::atomic<int> done{0};
    // copy (rows x bytes, pitches apart; a linear copy is one row), memset (dst, bytes, value)
    char* dst = nullptr;
    const char* src = nullptr;
    size_t bytes = 0, dpitch = 0, spitch = 0, rows = 1;
    int value = 0;
    bool checksummed = false;
    uint64_t sum = 0;
    bool caller_memory = false;  // reads or writes memory the model did not allocate for the library
    Op* bound = nullptr;         // wait: the record it waits for (nullptr: none, a no-op)
    const Hook* hook = nullptr;  // kernel
    std::vector<std::vector<char>> arg_copy;
    std::vector<void*> arg_ptr;
    std::vector<model_hip_range> writes;
};

struct StreamM {
    std::atomic<bool> alive{true};
    unsigned flags = 0;
    int index = 0;
    Op head;
    Op* tail = &head;  // (under pmu)
    Op* scan = &head;  // (under pmu) every op up to here is done
    std::mutex pmu;    // producers and scanners; never a worker
    Op* cur = &head;   // the last op executed: the worker's, or (eager, lazy) whoever holds xmu
    std::atomic<uint64_t> enq{0};
    uint64_t enq_base = 0;
    std::thread worker;
    std::atomic<bool> quit{false};
    uint64_t rng = 0;
    StreamM() { head.done.store(1); }
};

struct EventM {
    std::atomic<bool> alive{true};
    std::atomic<Op*> last{nullptr};  // the most recent record
};

struct Alloc {
    size_t bytes;
    bool device, caller;
};

struct Globals {
    int schedule = MODEL_HIP_EAGER;
    uint64_t seed = 1;
    int max_pause_us = 40;
    std::thread::id main_thread;
    std::recursive_mutex xmu;  // eager, lazy: whoever runs ops
    std::mutex rmu;            // the registry below
    std::map<uintptr_t, Alloc> allocs;
    std::set<uintptr_t> freed;
    std::map<uintptr_t, size_t> regs;  // page-rounded
    std::vector<StreamM*> streams;     // every stream ever made, in order
    std::set<EventM*> events;
    std::map<const void*, std::string> kernels;
    std::vector<Hook*> hooks;
    std::mutex emu;
    std::vector<std::string> errors;
    std::atomic<int> fail_memcpy{0}, fail_register{0}, refuse_every{0}, register_calls{0}, helper_pause{0}, registered_total{0};
};
Globals& G() {
    static Globals* g = new Globals();  // (never destroyed: module destructors of the library run after main)
    return *g;
}

thread_local hipError_t t_last_error = hipSuccess;
hipError_t fail(hipError_t e) {
    t_last_error = e;
    return e;
}

constexpr uintptr_t kPage = 4096;

uint64_t checksum(const char* p, size_t n, uint64_t h) {
    size_t i = 0;
    for (; i + 8 <= n; i += 8) {
        uint64_t w;
        std::memcpy(&w, p + i, 8);
        h = (h ^ w) * 0x9E3779B97F4A7C15ull;
        h ^= h >> 29;
    }
    for (; i < n; ++i) h = (h ^ (unsigned char)p[i]) * 0x100000001B3ull;
    return h;
}
uint64_t checksum_rows(const Op* op) {
    uint64_t h = 0xCBF29CE484222325ull;
    for (size_t r = 0; r < op->rows; ++r) h = checksum(op->src + r * op->spitch, op->bytes, h);
    return h;
}

// (under rmu) the allocation [p, p + n) lies in, or nullptr
const Alloc* alloc_of(const void* p, size_t n) {
    Globals& g = G();
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    auto it = g.allocs.upper_bound(a);
    if (it == g.allocs.begin()) return nullptr;
    --it;
    if (a >= it->first && a + n <= it->first + it->second.bytes) return &it->second;
    return nullptr;
}
bool device_range_ok(const void* p, size_t n, const char* what) {
    Globals& g = G();
    bool ok;
    {
        std::lock_guard<std::mutex> lk(g.rmu);
        const Alloc* a = alloc_of(p, n);
        ok = a && a->device;
    }
    if (!ok) model_hip_error("device-range", "%s: %zu bytes at %p do not lie inside one live device allocation", what, n, p);
    return ok;
}
// memory the model allocated for the library under test (not the caller's, not pageable, not registered)
bool library_memory(const void* p, size_t n) {
    Globals& g = G();
    std::lock_guard<std::mutex> lk(g.rmu);
    const Alloc* a = alloc_of(p, n);
    return a && !a->caller;
}
bool is_device(const void* p) {
    Globals& g = G();
    std::lock_guard<std::mutex> lk(g.rmu);
    const Alloc* a = alloc_of(p, 1);
    return a && a->device;
}

bool overlaps(const void* p, size_t n, const void* q, size_t m) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
    return n && m && a < b + m && b < a + n;
}
size_t span_of(size_t rows, size_t pitch, size_t bytes) { return rows ? (rows - 1) * pitch + bytes : 0; }
bool op_reads(const Op* op, const void* p, size_t n) {
    return op->kind == OP_COPY && overlaps(op->src, span_of(op->rows, op->spitch, op->bytes), p, n);
}
bool op_writes(const Op* op, const void* p, size_t n) {
    if (op->kind == OP_COPY || op->kind == OP_MEMSET) return overlaps(op->dst, span_of(op->rows, op->dpitch, op->bytes), p, n);
    if (op->kind == OP_KERNEL)
        for (const model_hip_range& r : op->writes)
            if (overlaps(r.p, r.bytes, p, n)) return true;
    return false;
}

// every op that is not known to be done, on every stream (the flag is read relaxed: this synchronises with nobody)
template <class F>
void for_pending(const F& f) {
    Globals& g = G();
    std::vector<StreamM*> ss;
    {
        std::lock_guard<std::mutex> lk(g.rmu);
        ss = g.streams;
    }
    for (StreamM* s : ss) {
        std::lock_guard<std::mutex> lk(s->pmu);
        for (Op* n; (n = s->scan->next.load(std::memory_order_acquire)) != nullptr && n->done.load(std::memory_order_relaxed);) s->scan = n;
        for (Op* n = s->scan->next.load(std::memory_order_acquire); n; n = n->next.load(std::memory_order_acquire))
            if (!n->done.load(std::memory_order_relaxed)) f(s, n);
    }
}

void execute(Op* op) {
    switch (op->kind) {
        case OP_COPY:
            if (op->checksummed && checksum_rows(op) != op->sum)
                model_hip_error("source-changed", "stream %d: the source of a pending transfer (%zu rows of %zu bytes at %p) changed between enqueue and execution",
                                op->stream->index, op->rows, op->bytes, (const void*)op->src);
            for (size_t r = 0; r < op->rows; ++r) std::memcpy(op->dst + r * op->dpitch, op->src + r * op->spitch, op->bytes);
            break;
        case OP_MEMSET: std::memset(op->dst, op->value, op->bytes); break;
        case OP_KERNEL:
            if (op->hook && op->hook->run) op->hook->run(op->hook->user, op->arg_ptr.data(), op->stream);
            break;
        default: break;
    }
    op->done.store(1, std::memory_order_release);
}

void idle(int& spins) {
    if (++spins < 100) std::this_thread::yield();
    else std::this_thread::sleep_for(std::chrono::microseconds(spins < 400 ? 20 : 100));
}

void worker_main(StreamM* s) {
    Globals& g = G();
    Op* cur = &s->head;
    int spins = 0;
    for (;;) {
        Op* n = cur->next.load(std::memory_order_acquire);
        if (!n) {
            if (s->quit.load(std::memory_order_acquire) && !cur->next.load(std::memory_order_acquire)) return;
            idle(spins);
            continue;
        }
        spins = 0;
        if (n->kind == OP_WAIT && n->bound)
            for (int sp = 0; !n->bound->done.load(std::memory_order_acquire);) idle(sp);
        if ((n->kind == OP_COPY || n->kind == OP_MEMSET || (n->kind == OP_KERNEL && n->hook)) && g.max_pause_us > 0) {
            s->rng = s->rng * 6364136223846793005ull + 1442695040888963407ull;
            const int us = (int)((s->rng >> 33) % (uint64_t)(g.max_pause_us + 1));
            if (us > 0) std::this_thread::sleep_for(std::chrono::microseconds(us));
        }
        execute(n);
        cur = n;
    }
}

// eager, lazy: run stream s up to and including `target`, and first whatever its waits are bound to
void force(StreamM* s, Op* target) {
    Globals& g = G();
    std::lock_guard<std::recursive_mutex> lk(g.xmu);
    while (!target->done.load(std::memory_order_relaxed)) {
        Op* n = s->cur->next.load(std::memory_order_acquire);
        if (!n) break;
        if (n->kind == OP_WAIT && n->bound && !n->bound->done.load(std::memory_order_relaxed)) force(n->bound->stream, n->bound);
        execute(n);
        s->cur = n;
    }
}

void sync_op(Op* target) {
    if (!target) return;
    if (G().schedule == MODEL_HIP_THREADED) {
        for (int sp = 0; !target->done.load(std::memory_order_acquire);) idle(sp);
    } else {
        force(target->stream, target);
    }
}
void sync_stream(StreamM* s) {
    Op* t;
    {
        std::lock_guard<std::mutex> lk(s->pmu);
        t = s->tail;
    }
    sync_op(t);
}
void sync_device(bool blocking_only) {
    Globals& g = G();
    std::vector<StreamM*> ss;
    {
        std::lock_guard<std::mutex> lk(g.rmu);
        ss = g.streams;
    }
    for (StreamM* s : ss)
        if (!blocking_only || !(s->flags & hipStreamNonBlocking)) sync_stream(s);
}

// (a record becomes its event's most recent one in the same step that puts it on the stream)
void enqueue(StreamM* s, Op* op, EventM* records = nullptr) {
    op->stream = s;
    {
        std::lock_guard<std::mutex> lk(s->pmu);
        s->tail->next.store(op, std::memory_order_release);
        s->tail = op;
        if (records) records->last.store(op, std::memory_order_release);
    }
    s->enq.fetch_add(1, std::memory_order_relaxed);
    if (G().schedule == MODEL_HIP_EAGER) force(s, op);
}

StreamM* null_stream() {
    static StreamM* s = [] {
        StreamM* n = new StreamM();
        n->index = -1;
        return n;
    }();
    return s;
}
// the stream behind a handle; nullptr (with the error recorded) if it was destroyed or never made
StreamM* stream_of(hipStream_t h, const char* what) {
    if (h == nullptr) return null_stream();
    Globals& g = G();
    StreamM* s = reinterpret_cast<StreamM*>(h);
    bool known;
    {
        std::lock_guard<std::mutex> lk(g.rmu);
        known = false;
        for (StreamM* k : g.streams) known = known || k == s;
    }
    if (!known || !s->alive.load()) {
        model_hip_error("destroyed-stream", "%s on a stream that %s", what, known ? "was destroyed" : "was never made");
        return nullptr;
    }
    return s;
}
EventM* event_of(hipEvent_t h, const char* what) {
    Globals& g = G();
    EventM* e = reinterpret_cast<EventM*>(h);
    bool known;
    {
        std::lock_guard<std::mutex> lk(g.rmu);
        known = g.events.count(e) != 0;
    }
    if (!known || !e->alive.load()) {
        model_hip_error("destroyed-event", "%s on an event that %s", what, known ? "was destroyed" : "was never made");
        return nullptr;
    }
    return e;
}
// async work on the null stream is not what the library does; run it at once
void after_enqueue(StreamM* s) {
    if (s == null_stream()) {
        sync_device(true);
        sync_stream(s);
    }
}

void helper_pause() {
    Globals& g = G();
    const int us = g.helper_pause.load(std::memory_order_relaxed);
    if (us > 0 && std::this_thread::get_id() != g.main_thread) std::this_thread::sleep_for(std::chrono::microseconds(us));
}
bool countdown(std::atomic<int>& c) {  // true on the call the switch named
    int v = c.load();
    while (v > 0)
        if (c.compare_exchange_weak(v, v - 1)) return v == 1;
    return false;
}

hipError_t copy_common(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t rows, hipMemcpyKind kind,
                       StreamM* s, const char* what) {
    if (width == 0 || rows == 0) return hipSuccess;
    bool src_dev = kind == hipMemcpyDeviceToHost || kind == hipMemcpyDeviceToDevice;
    bool dst_dev = kind == hipMemcpyHostToDevice || kind == hipMemcpyDeviceToDevice;
    if (kind == hipMemcpyDefault) {
        src_dev = is_device(src);
        dst_dev = is_device(dst);
    }
    bool ok = true;
    if (src_dev) ok = device_range_ok(src, span_of(rows, spitch, width), what) && ok;
    if (dst_dev) ok = device_range_ok(dst, span_of(rows, dpitch, width), what) && ok;
    if (!ok) return fail(hipErrorInvalidValue);
    Op* op = new Op();
    op->kind = OP_COPY;
    op->dst = static_cast<char*>(dst);
    op->src = static_cast<const char*>(src);
    op->bytes = width;
    op->dpitch = dpitch;
    op->spitch = spitch;
    op->rows = rows;
    op->caller_memory = (!src_dev && !library_memory(src, span_of(rows, spitch, width))) || (!dst_dev && !library_memory(dst, span_of(rows, dpitch, width)));
    if (!src_dev) {
        op->checksummed = true;
        op->sum = checksum_rows(op);
    }
    if (s) {
        enqueue(s, op);
        after_enqueue(s);
    } else {
        // a blocking copy: the null stream's, which waits for blocking streams only
        sync_device(true);
        for_pending([&](StreamM* ps, Op* p) {
            if (op_writes(p, src, span_of(rows, spitch, width)))
                model_hip_error("blocking-copy-unwritten", "%s reads %zu bytes at %p that a pending op of stream %d has yet to write (the stream is non-blocking: the copy does not wait for it)",
                                what, span_of(rows, spitch, width), src, ps->index);
        });
        op->stream = null_stream();
        execute(op);
        delete op;
    }
    return hipSuccess;
}

}  // namespace

// ---- control ---------------------------------------------------------------------------------------------------------------

extern "C" {

void model_hip_init(int schedule, uint64_t seed, int max_pause_us) {
    Globals& g = G();
    g.schedule = schedule;
    g.seed = seed;
    g.max_pause_us = max_pause_us;
    g.main_thread = std::this_thread::get_id();
}

void model_hip_hook(const char* name_part, int n_args, const size_t* arg_bytes, model_hip_kernel_run run, model_hip_kernel_writes writes,
                    void* user) {
    Globals& g = G();
    Hook* h = new Hook{name_part, std::vector<size_t>(arg_bytes, arg_bytes + n_args), run, writes, user};
    std::lock_guard<std::mutex> lk(g.rmu);
    g.hooks.push_back(h);
}

void model_hip_error(const char* rule, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    Globals& g = G();
    std::lock_guard<std::mutex> lk(g.emu);
    if (g.errors.size() < 200) g.errors.push_back(std::string("[") + rule + "] " + buf);
}
int model_hip_error_count(void) {
    Globals& g = G();
    std::lock_guard<std::mutex> lk(g.emu);
    return (int)g.errors.size();
}
void model_hip_print_errors(void) {
    Globals& g = G();
    std::lock_guard<std::mutex> lk(g.emu);
    for (const std::string& e : g.errors) std::fprintf(stderr, "model_hip: %s\n", e.c_str());
}
void model_hip_clear_errors(void) {
    Globals& g = G();
    std::lock_guard<std::mutex> lk(g.emu);
    g.errors.clear();
}

void model_hip_mark_caller_memory(const void* p) {
    Globals& g = G();
    std::lock_guard<std::mutex> lk(g.rmu);
    auto it = g.allocs.find(reinterpret_cast<uintptr_t>(p));
    if (it != g.allocs.end()) it->second.caller = true;
}
void model_hip_check_quiescent(void) {
    for_pending([&](StreamM* s, Op* p) {
        if (p->caller_memory)
            model_hip_error("caller-memory-pending", "stream %d: a transfer of %zu rows of %zu bytes (%p -> %p) is still pending on the caller's memory",
                            s->index, p->rows, p->bytes, (const void*)p->src, (void*)p->dst);
    });
}
void model_hip_drain(void) { sync_device(false); }
int model_hip_pending_work(void) {
    int n = 0;
    for_pending([&](StreamM*, Op* p) { n += (p->kind == OP_COPY || p->kind == OP_MEMSET || p->kind == OP_KERNEL) ? 1 : 0; });
    return n;
}
void model_hip_check_leaks(void) {
    Globals& g = G();
    size_t a, r, s = 0, e = 0;
    {
        std::lock_guard<std::mutex> lk(g.rmu);
        a = g.allocs.size();
        r = g.regs.size();
        for (StreamM* k : g.streams) s += k->alive.load() ? 1 : 0;
        for (EventM* k : g.events) e += k->alive.load() ? 1 : 0;
    }
    if (a || r || s || e) model_hip_error("leak", "at exit: %zu allocations, %zu registered ranges, %zu streams, %zu events are still live", a, r, s, e);
}

void model_hip_fail_memcpy_async_at(int nth) { G().fail_memcpy.store(nth); }
void model_hip_fail_host_register_at(int nth) { G().fail_register.store(nth); }
void model_hip_refuse_register_every(int k) {
    G().refuse_every.store(k);
    G().register_calls.store(0);
}
void model_hip_helper_pause_us(int us) { G().helper_pause.store(us); }

int model_hip_trace_lengths(uint64_t* out, int cap) {
    Globals& g = G();
    std::lock_guard<std::mutex> lk(g.rmu);
    int n = 0;
    for (StreamM* s : g.streams) {
        if (!s->alive.load()) continue;
        if (n < cap) out[n] = s->enq.load() - s->enq_base;
        ++n;
    }
    return n;
}
void model_hip_reset_counters(void) {
    Globals& g = G();
    std::lock_guard<std::mutex> lk(g.rmu);
    for (StreamM* s : g.streams) s->enq_base = s->enq.load();
    g.registered_total.store(0);
}
int model_hip_registered_total(void) { return G().registered_total.load(); }
int model_hip_registered_ranges(void) {
    Globals& g = G();
    std::lock_guard<std::mutex> lk(g.rmu);
    return (int)g.regs.size();
}

// ---- the launch plumbing ---------------------------------------------------------------------------------------------------

static void* g_fatbin_handle[1];
void** __hipRegisterFatBinary(const void*) { return g_fatbin_handle; }
void __hipUnregisterFatBinary(void**) {}
void __hipRegisterFunction(void**, const void* host_fn, char*, const char* device_name, unsigned, void*, void*, void*, void*, int*) {
    Globals& g = G();
    std::lock_guard<std::mutex> lk(g.rmu);
    g.kernels[host_fn] = device_name ? device_name : "";
}
void __hipRegisterVar(void**, void*, char*, const char*, int, size_t, int, int) {}

struct CallConfig {
    dim3 grid, block;
    size_t shmem;
    hipStream_t stream;
};
static thread_local std::vector<CallConfig> t_config;
hipError_t __hipPushCallConfiguration(dim3 grid, dim3 block, size_t shmem, hipStream_t stream) {
    t_config.push_back(CallConfig{grid, block, shmem, stream});
    return hipSuccess;
}
hipError_t __hipPopCallConfiguration(dim3* grid, dim3* block, size_t* shmem, hipStream_t* stream) {
    if (t_config.empty()) return fail(hipErrorInvalidConfiguration);
    const CallConfig c = t_config.back();
    t_config.pop_back();
    *grid = c.grid;
    *block = c.block;
    *shmem = c.shmem;
    *stream = c.stream;
    return hipSuccess;
}

hipError_t hipLaunchKernel(const void* fn, dim3, dim3, void** args, size_t, hipStream_t stream) {
    Globals& g = G();
    StreamM* s = stream_of(stream, "hipLaunchKernel");
    if (!s) return fail(hipErrorInvalidHandle);
    const Hook* hook = nullptr;
    {
        std::lock_guard<std::mutex> lk(g.rmu);
        auto it = g.kernels.find(fn);
        if (it == g.kernels.end()) {
            model_hip_error("unknown-kernel", "hipLaunchKernel of a function that was never registered");
            return fail(hipErrorInvalidDeviceFunction);
        }
        for (const Hook* h : g.hooks)
            if (it->second.find(h->part) != std::string::npos) hook = h;
    }
    Op* op = new Op();
    op->kind = OP_KERNEL;
    op->hook = hook;
    if (hook) {
        op->arg_copy.resize(hook->arg_bytes.size());
        for (size_t i = 0; i < hook->arg_bytes.size(); ++i) {
            op->arg_copy[i].assign(static_cast<const char*>(args[i]), static_cast<const char*>(args[i]) + hook->arg_bytes[i]);
            op->arg_ptr.push_back(op->arg_copy[i].data());
        }
        if (hook->writes) {
            model_hip_range r[8];
            const int n = hook->writes(hook->user, op->arg_ptr.data(), r, 8);
            op->writes.assign(r, r + n);
        }
    }
    enqueue(s, op);
    after_enqueue(s);
    return hipSuccess;
}

// ---- device, errors ---------------------------------------------------------------------------------------------------------

hipError_t hipGetDeviceCount(int* n) {
    *n = 1;
    return hipSuccess;
}
hipError_t hipSetDevice(int d) { return d == 0 ? hipSuccess : fail(hipErrorInvalidDevice); }
hipError_t hipGetDevice(int* d) {
    *d = 0;
    return hipSuccess;
}
hipError_t hipDeviceGetStreamPriorityRange(int* lo, int* hi) {
    *lo = 0;
    *hi = -1;
    return hipSuccess;
}
hipError_t hipDeviceGetPCIBusId(char*, int, int) { return fail(hipErrorInvalidDevice); }  // (no NUMA node to bind to)
hipError_t hipFuncSetAttribute(const void*, hipFuncAttribute, int) { return hipSuccess; }
hipError_t hipGetLastError(void) {
    const hipError_t e = t_last_error;
    t_last_error = hipSuccess;
    return e;
}
const char* hipGetErrorString(hipError_t e) {
    switch (e) {
        case hipSuccess: return "no error";
        case hipErrorInvalidValue: return "invalid argument";
        case hipErrorOutOfMemory: return "out of memory";
        case hipErrorHostMemoryAlreadyRegistered: return "part or all of the requested memory range is already mapped";
        case hipErrorHostMemoryNotRegistered: return "pointer does not correspond to a registered memory region";
        case hipErrorUnknown: return "unknown error (injected by the model)";
        default: return "error (model runtime)";
    }
}

// ---- memory -----------------------------------------------------------------------------------------------------------------

static hipError_t model_alloc(void** out, size_t bytes, bool device) {
    Globals& g = G();
    void* p = nullptr;
    if (posix_memalign(&p, kPage, bytes ? bytes : 1) != 0) return fail(hipErrorOutOfMemory);
    std::memset(p, 0, bytes);
    std::lock_guard<std::mutex> lk(g.rmu);
    g.allocs[reinterpret_cast<uintptr_t>(p)] = Alloc{bytes, device, false};
    g.freed.erase(reinterpret_cast<uintptr_t>(p));
    *out = p;
    return hipSuccess;
}
static hipError_t model_free(void* p, bool device, const char* what) {
    if (!p) return hipSuccess;
    Globals& g = G();
    sync_device(false);  // (as HIP does)
    size_t bytes = 0;
    bool found = false, twice = false;
    {
        std::lock_guard<std::mutex> lk(g.rmu);
        auto it = g.allocs.find(reinterpret_cast<uintptr_t>(p));
        found = it != g.allocs.end() && it->second.device == device;
        if (found) bytes = it->second.bytes;
        else twice = g.freed.count(reinterpret_cast<uintptr_t>(p)) != 0;
    }
    if (!found) {
        if (twice) model_hip_error("double-free", "%s of %p, which was freed already", what, p);
        else model_hip_error("free-unknown", "%s of %p, which this call cannot free", what, p);
        return fail(hipErrorInvalidValue);
    }
    for_pending([&](StreamM* s, Op* o) {
        if (op_reads(o, p, bytes) || op_writes(o, p, bytes))
            model_hip_error("free-pending", "%s of %zu bytes at %p that a pending op of stream %d still touches", what, bytes, p, s->index);
    });
    {
        std::lock_guard<std::mutex> lk(g.rmu);
        g.allocs.erase(reinterpret_cast<uintptr_t>(p));
        g.freed.insert(reinterpret_cast<uintptr_t>(p));
    }
    std::free(p);
    return hipSuccess;
}
hipError_t hipMalloc(void** p, size_t bytes) { return model_alloc(p, bytes, true); }
hipError_t hipFree(void* p) { return model_free(p, true, "hipFree"); }
hipError_t hipHostMalloc(void** p, size_t bytes, unsigned) { return model_alloc(p, bytes, false); }
hipError_t hipHostFree(void* p) { return model_free(p, false, "hipHostFree"); }

hipError_t hipHostRegister(void* p, size_t bytes, unsigned) {
    Globals& g = G();
    if (countdown(g.fail_register)) return fail(hipErrorUnknown);
    const int every = g.refuse_every.load();
    if (every > 0 && (g.register_calls.fetch_add(1) + 1) % every == 0) return fail(hipErrorHostMemoryAlreadyRegistered);
    const uintptr_t lo = reinterpret_cast<uintptr_t>(p) & ~(kPage - 1), hi = (reinterpret_cast<uintptr_t>(p) + bytes + kPage - 1) & ~(kPage - 1);
    bool twice = false;
    {
        std::lock_guard<std::mutex> lk(g.rmu);
        for (const auto& r : g.regs) twice = twice || (lo < r.first + r.second && r.first < hi);
        if (alloc_of(p, 1)) twice = true;  // (page-locked by the runtime already)
        if (!twice) g.regs[lo] = hi - lo;
        if (!twice) g.registered_total.fetch_add(1);
    }
    if (twice) {
        model_hip_error("register-twice", "hipHostRegister of %zu bytes at %p: a page of the range is page-locked already", bytes, p);
        return fail(hipErrorHostMemoryAlreadyRegistered);
    }
    return hipSuccess;
}
hipError_t hipHostUnregister(void* p) {
    Globals& g = G();
    const uintptr_t lo = reinterpret_cast<uintptr_t>(p) & ~(kPage - 1);
    size_t bytes = 0;
    {
        std::lock_guard<std::mutex> lk(g.rmu);
        auto it = g.regs.find(lo);
        if (it != g.regs.end()) bytes = it->second;
    }
    if (!bytes) {
        model_hip_error("unregister-unknown", "hipHostUnregister of %p, which is not registered", p);
        return fail(hipErrorHostMemoryNotRegistered);
    }
    for_pending([&](StreamM* s, Op* o) {
        if (op_reads(o, reinterpret_cast<void*>(lo), bytes) || op_writes(o, reinterpret_cast<void*>(lo), bytes))
            model_hip_error("unregister-pending", "hipHostUnregister of %p under a pending transfer of stream %d", p, s->index);
    });
    std::lock_guard<std::mutex> lk(g.rmu);
    g.regs.erase(lo);
    return hipSuccess;
}
hipError_t hipPointerGetAttributes(hipPointerAttribute_t* a, const void* p) {
    Globals& g = G();
    std::lock_guard<std::mutex> lk(g.rmu);
    std::memset(a, 0, sizeof(*a));
    if (const Alloc* al = alloc_of(p, 1)) {
        a->type = al->device ? hipMemoryTypeDevice : hipMemoryTypeHost;
        return hipSuccess;
    }
    const uintptr_t x = reinterpret_cast<uintptr_t>(p);
    for (const auto& r : g.regs)
        if (x >= r.first && x < r.first + r.second) {
            a->type = hipMemoryTypeHost;
            return hipSuccess;
        }
    return fail(hipErrorInvalidValue);
}

hipError_t hipMemcpy(void* dst, const void* src, size_t n, hipMemcpyKind kind) { return copy_common(dst, n, src, n, n, 1, kind, nullptr, "hipMemcpy"); }
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t n, hipMemcpyKind kind, hipStream_t stream) {
    helper_pause();
    if (countdown(G().fail_memcpy)) return fail(hipErrorUnknown);
    StreamM* s = stream_of(stream, "hipMemcpyAsync");
    if (!s) return fail(hipErrorInvalidHandle);
    return copy_common(dst, n, src, n, n, 1, kind, s, "hipMemcpyAsync");
}
hipError_t hipMemcpy2DAsync(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t height, hipMemcpyKind kind,
                            hipStream_t stream) {
    StreamM* s = stream_of(stream, "hipMemcpy2DAsync");
    if (!s) return fail(hipErrorInvalidHandle);
    if (dpitch < width || spitch < width) return fail(hipErrorInvalidPitchValue);
    return copy_common(dst, dpitch, src, spitch, width, height, kind, s, "hipMemcpy2DAsync");
}
static hipError_t memset_common(void* dst, int value, size_t n, StreamM* s, const char* what) {
    if (n == 0) return hipSuccess;
    if (!device_range_ok(dst, n, what)) return fail(hipErrorInvalidValue);
    Op* op = new Op();
    op->kind = OP_MEMSET;
    op->dst = static_cast<char*>(dst);
    op->bytes = op->dpitch = n;
    op->value = value;
    if (s) {
        enqueue(s, op);
        after_enqueue(s);
    } else {
        sync_device(true);
        op->stream = null_stream();
        execute(op);
        delete op;
    }
    return hipSuccess;
}
hipError_t hipMemset(void* dst, int value, size_t n) { return memset_common(dst, value, n, nullptr, "hipMemset"); }
hipError_t hipMemsetAsync(void* dst, int value, size_t n, hipStream_t stream) {
    StreamM* s = stream_of(stream, "hipMemsetAsync");
    if (!s) return fail(hipErrorInvalidHandle);
    return memset_common(dst, value, n, s, "hipMemsetAsync");
}

// ---- streams and events -----------------------------------------------------------------------------------------------------

hipError_t hipStreamCreateWithPriority(hipStream_t* out, unsigned flags, int) {
    Globals& g = G();
    StreamM* s = new StreamM();
    s->flags = flags;
    {
        std::lock_guard<std::mutex> lk(g.rmu);
        s->index = (int)g.streams.size();
        g.streams.push_back(s);
    }
    s->rng = (g.seed + 0x9E3779B97F4A7C15ull * (uint64_t)(s->index + 1)) | 1ull;
    if (g.schedule == MODEL_HIP_THREADED) s->worker = std::thread(worker_main, s);
    *out = reinterpret_cast<hipStream_t>(s);
    return hipSuccess;
}
hipError_t hipStreamCreateWithFlags(hipStream_t* out, unsigned flags) { return hipStreamCreateWithPriority(out, flags, 0); }
hipError_t hipStreamDestroy(hipStream_t h) {
    StreamM* s = stream_of(h, "hipStreamDestroy");
    if (!s || s == null_stream()) return fail(hipErrorInvalidHandle);
    sync_stream(s);  // (HIP lets the stream's work finish; so does the model, here)
    s->alive.store(false);
    if (s->worker.joinable()) {
        s->quit.store(true, std::memory_order_release);
        s->worker.join();
    }
    return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t h) {
    StreamM* s = stream_of(h, "hipStreamSynchronize");
    if (!s) return fail(hipErrorInvalidHandle);
    if (s == null_stream()) sync_device(true);
    sync_stream(s);
    return hipSuccess;
}
hipError_t hipDeviceSynchronize(void) {
    sync_device(false);
    return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t* out, unsigned) {
    Globals& g = G();
    EventM* e = new EventM();
    std::lock_guard<std::mutex> lk(g.rmu);
    g.events.insert(e);
    *out = reinterpret_cast<hipEvent_t>(e);
    return hipSuccess;
}
hipError_t hipEventCreate(hipEvent_t* out) { return hipEventCreateWithFlags(out, 0); }
hipError_t hipEventDestroy(hipEvent_t h) {
    EventM* e = event_of(h, "hipEventDestroy");
    if (!e) return fail(hipErrorInvalidHandle);
    e->alive.store(false);
    return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t h, hipStream_t stream) {
    helper_pause();
    EventM* e = event_of(h, "hipEventRecord");
    StreamM* s = stream_of(stream, "hipEventRecord");
    if (!e || !s) return fail(hipErrorInvalidHandle);
    Op* op = new Op();
    op->kind = OP_RECORD;
    enqueue(s, op, e);
    after_enqueue(s);
    return hipSuccess;
}
hipError_t hipStreamWaitEvent(hipStream_t stream, hipEvent_t h, unsigned) {
    EventM* e = event_of(h, "hipStreamWaitEvent");
    StreamM* s = stream_of(stream, "hipStreamWaitEvent");
    if (!e || !s) return fail(hipErrorInvalidHandle);
    Op* op = new Op();
    op->kind = OP_WAIT;
    op->bound = e->last.load(std::memory_order_acquire);  // the most recent record NOW; none: a no-op
    enqueue(s, op);
    after_enqueue(s);
    return hipSuccess;
}
hipError_t hipEventSynchronize(hipEvent_t h) {
    EventM* e = event_of(h, "hipEventSynchronize");
    if (!e) return fail(hipErrorInvalidHandle);
    sync_op(e->last.load(std::memory_order_acquire));
    return hipSuccess;
}
hipError_t hipEventElapsedTime(float* ms, hipEvent_t a, hipEvent_t b) {
    EventM* ea = event_of(a, "hipEventElapsedTime");
    EventM* eb = event_of(b, "hipEventElapsedTime");
    *ms = 0.f;
    if (!ea || !eb) return fail(hipErrorInvalidHandle);
    Op* ra = ea->last.load(std::memory_order_acquire);
    Op* rb = eb->last.load(std::memory_order_acquire);
    if (!ra || !rb) return fail(hipErrorInvalidHandle);
    if (!ra->done.load(std::memory_order_acquire) || !rb->done.load(std::memory_order_acquire)) return fail(hipErrorNotReady);
    return hipSuccess;
}

}  // extern "C"
