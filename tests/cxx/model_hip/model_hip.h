// Control interface of the model HIP runtime (model_hip.cpp): what a test harness needs beside the HIP entry points
// themselves.  The model is written from HIP's documented stream, event and memory semantics; it knows nothing of the
// library that is linked against it.
#pragma once
#include <cstddef>
#include <cstdint>

extern "C" {

// How enqueued ops run.
//   eager:    an op runs when it is enqueued (the baseline: proves the harness's own expectations)
//   lazy:     an op runs only when a synchronising call forces it, i.e. at the last moment HIP's rules allow
//             (deterministic, no thread of the model's own)
//   threaded: one worker per stream, a seeded pseudo-random pause in front of every op; the only happens-before edges
//             from a worker to a host thread are the model's synchronising calls, so a missing dependency is a data race
enum model_hip_schedule { MODEL_HIP_EAGER = 0, MODEL_HIP_LAZY = 1, MODEL_HIP_THREADED = 2 };
// (before the first HIP call of the process; max_pause_us: upper bound of a worker's pause)
void model_hip_init(int schedule, uint64_t seed, int max_pause_us);

// A memory range a kernel will write (for the "blocking copy out of a range yet to be written" rule).
struct model_hip_range {
    const void* p;
    size_t bytes;
};
// Behaviour of the kernels whose registered (mangled) name contains `name_part`: `run` is called when the model executes
// a launch, with copies of the launch's arguments (args[i] points at a copy of argument i, arg_bytes[i] long).  `writes`
// (optional) names up to `cap` ranges the launch will write and returns how many.  Kernels without a behaviour do nothing.
typedef void (*model_hip_kernel_run)(void* user, void* const* args, void* stream);
typedef int (*model_hip_kernel_writes)(void* user, void* const* args, model_hip_range* out, int cap);
void model_hip_hook(const char* name_part, int n_args, const size_t* arg_bytes, model_hip_kernel_run run,
                    model_hip_kernel_writes writes, void* user);

// Errors: the model records one line per violated rule, "[rule-name] details".  The harness may add its own.
void model_hip_error(const char* rule, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
int model_hip_error_count(void);
void model_hip_print_errors(void);  // to stderr
void model_hip_clear_errors(void);

// Memory of the model's hipHostMalloc that belongs to the CALLER of the library under test (a page-locked frame), so that
// model_hip_check_quiescent counts it as the caller's, like registered and pageable memory.
void model_hip_mark_caller_memory(const void* p);
// Records [caller-memory-pending] for every pending op that reads or writes memory the model did not allocate for the
// library (pageable, registered, or marked above).  Runs nothing.
void model_hip_check_quiescent(void);
// Copies, memsets and launches that are still pending, on all streams together (event records and waits do not count).
int model_hip_pending_work(void);
// Runs everything that is pending on every stream (what hipDeviceSynchronize does).
void model_hip_drain(void);
// After every context is destroyed: records [leak] for live allocations, registered ranges, streams and events.
void model_hip_check_leaks(void);

// Switches.  The n-th call from now (1 = the next) of the named entry point fails (0: none).
void model_hip_fail_memcpy_async_at(int nth);
void model_hip_fail_host_register_at(int nth);
void model_hip_refuse_register_every(int k);  // every k-th hipHostRegister is refused (0: none)
// hipEventRecord and hipMemcpyAsync called from a thread other than `main_thread_only`'s pause this long first: lets a
// harness make the library's helper threads slower than its driving thread, deterministically
void model_hip_helper_pause_us(int us);

// Counters since the last model_hip_reset_counters: ops enqueued per live stream (in order of creation; the function returns
// how many live streams there are), ranges registered since then; and the ranges registered right now.
int model_hip_trace_lengths(uint64_t* out, int cap);
void model_hip_reset_counters(void);
int model_hip_registered_total(void);
int model_hip_registered_ranges(void);
}
