// lfm_farm.hip — the RCCL result farm behind include/lfm.h (lfm_farm_*): the communicator, the
// host-staged all-gather and the device-side round of a resident batch (enqueued, or replayed as
// one captured graph).
// librccl is opened lazily so the library loads (and the CPU tests run) without it.
#include <dlfcn.h>
#include <rccl/rccl.h>
#include <unistd.h>

#include <chrono>
#include <cstdio>
#include <cstring>
#include <ctime>

#include "lfm_api_internal.h"

using namespace lfm;

namespace {
// (both kernels keep their plain C names, as profiles and traces know them)
// Holds its stream for `ticks` of the 100 MHz constant clock, then exits (one wave).
extern "C" __global__ void stall_kernel(unsigned long long ticks) {
  const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
  while (__builtin_amdgcn_s_memrealtime() - t0 < ticks) __builtin_amdgcn_s_sleep(127);
}

// The end of a device-side farm round: the gathered slots to pinned host memory, then the round's
// sequence number — the host's completion signal (it spins on that word instead of synchronising
// the stream: microseconds sooner). ONE wave (launched with 64 threads): the sequence word's
// system-scope release store waits for every store the wave issued before it (s_waitcnt
// vmcnt(0) is per wave) after the L2 write-back, so the slots land first; a per-thread
// __threadfence_system before it would only repeat that write-back.
extern "C" __global__ __launch_bounds__(64) void farm_publish_kernel(
    const double* __restrict__ src, int64_t count, double* __restrict__ dst, unsigned* seq_word,
    unsigned seq) {
  for (int64_t i = threadIdx.x; i < count; i += 64) dst[i] = src[i];
  __syncthreads();
  if (threadIdx.x == 0)
    __hip_atomic_store(seq_word, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

struct Rccl {
  void* h = nullptr;
  ncclResult_t (*getUniqueId)(ncclUniqueId*) = nullptr;
  ncclResult_t (*commInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*allGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t,
                            hipStream_t) = nullptr;
  ncclResult_t (*commDestroy)(ncclComm_t) = nullptr;
  const char* (*errStr)(ncclResult_t) = nullptr;
  // optional (non-blocking communicator, bounded waits): absent -> blocking init
  ncclResult_t (*commInitRankConfig)(ncclComm_t*, int, ncclUniqueId, int, ncclConfig_t*) = nullptr;
  ncclResult_t (*commGetAsyncError)(ncclComm_t, ncclResult_t*) = nullptr;
  ncclResult_t (*commAbort)(ncclComm_t) = nullptr;
};
Rccl g_rccl;

int rccl_load(lfm_ctx* ctx) {
  if (g_rccl.h) return LFM_OK;
  void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
  if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
  if (!h) return set_err(ctx, LFM_E_RCCL, std::string("dlopen librccl: ") + dlerror());
  g_rccl.getUniqueId = (decltype(g_rccl.getUniqueId))dlsym(h, "ncclGetUniqueId");
  g_rccl.commInitRank = (decltype(g_rccl.commInitRank))dlsym(h, "ncclCommInitRank");
  g_rccl.allGather = (decltype(g_rccl.allGather))dlsym(h, "ncclAllGather");
  g_rccl.commDestroy = (decltype(g_rccl.commDestroy))dlsym(h, "ncclCommDestroy");
  g_rccl.errStr = (decltype(g_rccl.errStr))dlsym(h, "ncclGetErrorString");
  g_rccl.commInitRankConfig =
      (decltype(g_rccl.commInitRankConfig))dlsym(h, "ncclCommInitRankConfig");
  g_rccl.commGetAsyncError = (decltype(g_rccl.commGetAsyncError))dlsym(h, "ncclCommGetAsyncError");
  g_rccl.commAbort = (decltype(g_rccl.commAbort))dlsym(h, "ncclCommAbort");
  if (!g_rccl.getUniqueId || !g_rccl.commInitRank || !g_rccl.allGather || !g_rccl.commDestroy)
    return set_err(ctx, LFM_E_RCCL, "librccl lacks a required symbol");
  g_rccl.h = h;
  return LFM_OK;
}

int rccl_fail(lfm_ctx* ctx, ncclResult_t r, const char* what) {
  if (r == ncclSuccess) return LFM_OK;
  return set_err(ctx, LFM_E_RCCL,
                 std::string(what) + ": " + (g_rccl.errStr ? g_rccl.errStr(r) : "rccl error"));
}

// Bound on every wait of a non-blocking communicator (seconds, LFM_RCCL_TIMEOUT_S at context
// creation, default 300): a peer rank that died or never joined ends the call with LFM_E_RCCL
// instead of a hang.
double rccl_timeout_s(const lfm_ctx* ctx) { return ctx->knobs.rccl_timeout_s; }

double mono_s() {
  timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

// Waiting on a latency-bound exchange (a 16-256 B all-gather takes tens of microseconds over
// xGMI): poll tightly for the first 2 ms, then back off to 20 us sleeps, and to 200 us past
// 100 ms (a peer still initialising, or one that never arrives before the deadline).
struct Backoff {
  double t0 = mono_s();
  void pause() const {
    const double el = mono_s() - t0;
    if (el < 2e-3) return;  // spin: the next poll follows at once
    usleep(el < 0.1 ? 20 : 200);
  }
};

// Forget the captured farm round (its buffers, batch or communicator are changing; nothing of it
// is in flight).
void farm_graph_reset(lfm_ctx* ctx) {
  if (ctx->farm_exec) hipGraphExecDestroy(ctx->farm_exec);
  ctx->farm_exec = nullptr;
  ctx->farm_exec_batch = 0;
}

// End a communicator after a failed or timed-out operation: ncclCommAbort (a non-blocking
// communicator's pending kernels are released), and the context forgets it.
// Work the aborted call left queued on the stream (its copies into the farm's pinned staging,
// its publish kernel) may still run: farm_stale makes the next call drain it first (bounded), and
// abandon the staging buffers if it does not drain (a bounded leak instead of a late write into
// memory the next call is using).
void rccl_drop(lfm_ctx* ctx) {
  // a replay of the captured round may still be queued: the graph is set aside and destroyed
  // only once the stream has drained (farm_drain_stale; a second abort before that leaks one)
  if (ctx->farm_exec) {
    ctx->farm_exec_old = ctx->farm_exec;
    ctx->farm_exec = nullptr;
    ctx->farm_exec_batch = 0;
  }
  if (!ctx->comm) return;
  if (g_rccl.commAbort) g_rccl.commAbort((ncclComm_t)ctx->comm);
  else if (g_rccl.commDestroy) g_rccl.commDestroy((ncclComm_t)ctx->comm);
  ctx->comm = nullptr;
  ctx->nranks = 0;
  ctx->rank = -1;
  ctx->farm_stale = true;
}

// Poll a non-blocking communicator until its pending operation leaves ncclInProgress.
int rccl_poll(lfm_ctx* ctx, ncclComm_t comm, const char* what) {
  const double end = mono_s() + rccl_timeout_s(ctx);
  const Backoff bo;
  for (;;) {
    ncclResult_t st = ncclInProgress;
    const ncclResult_t q = g_rccl.commGetAsyncError(comm, &st);
    if (q != ncclSuccess) return rccl_fail(ctx, q, what);
    if (st != ncclInProgress) return rccl_fail(ctx, st, what);
    if (mono_s() > end)
      return set_err(ctx, LFM_E_RCCL, std::string(what) + ": timed out (a peer rank did not join)");
    bo.pause();
  }
}

// Bounded wait for everything enqueued on the context's stream (the collective included): a
// collective whose peers never arrive would otherwise block the stream, and the caller, forever.
int rccl_stream_wait(lfm_ctx* ctx, const char* what) {
  const double end = mono_s() + rccl_timeout_s(ctx);
  const Backoff bo;
  hipError_t e;
  while ((e = hipStreamQuery(ctx->stream)) == hipErrorNotReady) {
    const double now = mono_s();
    if (now > end) {
      char waited[64];
      std::snprintf(waited, sizeof(waited), " after %.2f s", now - bo.t0);
      return set_err(ctx, LFM_E_RCCL,
                     std::string(what) + ": timed out" + waited + " (a peer rank did not arrive)");
    }
    bo.pause();
  }
  return hip_fail(ctx, e, what);
}

// Enqueue the all-gather of `n` doubles per rank (dsend -> drecv, device).
int farm_allgather(lfm_ctx* ctx, const double* dsend, double* drecv, int64_t n) {
  // test instrument: a collective whose peers are late, stood in for by a kernel that holds
  // the stream for LFM_DEBUG_FARM_STALL_MS (the one-GPU box cannot host a second rank)
  if (const int stall = ctx->knobs.farm_stall_ms)
    hipLaunchKernelGGL(stall_kernel, dim3(1), dim3(64), 0, ctx->stream,
                       (unsigned long long)stall * 100000ull);
  const ncclResult_t q =
      g_rccl.allGather(dsend, drecv, (size_t)n, ncclFloat64, (ncclComm_t)ctx->comm, ctx->stream);
  return ctx->comm_nb && q == ncclInProgress ? rccl_poll(ctx, (ncclComm_t)ctx->comm, "ncclAllGather")
                                             : rccl_fail(ctx, q, "ncclAllGather");
}

// Before a farm call writes its host staging: work a dropped (timed-out) call left queued is
// drained, within the communicator's time bound; if it does not drain, the staging buffers it
// could still write are abandoned (never freed, never reused) and fresh ones are made.
int farm_drain_stale(lfm_ctx* ctx) {
  if (!ctx->farm_stale) return LFM_OK;
  const double end = mono_s() + std::min(rccl_timeout_s(ctx), 5.0);
  const Backoff bo;
  hipError_t e;
  while ((e = hipStreamQuery(ctx->stream)) == hipErrorNotReady && mono_s() < end) bo.pause();
  if (e == hipErrorNotReady) {
    farm_graph_reset(ctx);
    ctx->farm_h.abandon();  // abandoned: a queued copy may still land in it
    ctx->farm_pub.abandon();
    ctx->farm_buf.abandon();  // (device) the same for the queued collective's buffers
  } else if (e != hipSuccess) {
    return hip_fail(ctx, e, "draining the aborted farm call");
  } else if (ctx->farm_exec_old) {
    hipGraphExecDestroy(ctx->farm_exec_old);
    ctx->farm_exec_old = nullptr;
  }
  ctx->farm_stale = false;
  return LFM_OK;
}

// The all-gather's device buffer, send | recv, grown to `bytes`.
int farm_device_buffer(lfm_ctx* ctx, size_t bytes) {
  const double* before = ctx->farm_buf;
  int r = ctx->farm_buf.reserve(ctx, bytes);
  if (r) return r;
  // the captured farm round holds the old device buffer's addresses: forget it
  if (ctx->farm_buf != before) farm_graph_reset(ctx);
  return LFM_OK;
}

// The device-side round's buffers: send [slots] | recv [nranks slots] on the device, the
// publish target (recv's copy + a sequence word) in coherent pinned host memory.
int farm_buffers(lfm_ctx* ctx, size_t slots) {
  const size_t in = slots * 8, out = in * ctx->nranks;
  int r = farm_device_buffer(ctx, in + out);
  if (r) return r;
  const size_t pub = out + 64;
  if (!ctx->farm_pub || ctx->farm_pub.bytes < pub) {
    farm_graph_reset(ctx);
    r = ctx->farm_pub.reserve(ctx, pub, hipHostMallocCoherent, "farm publish buffer");
  }
  return r;
}

// The host's side of a device-side round: wait (bounded) for the publish kernel's sequence word,
// then copy the gathered slots out; on a fault or timeout the communicator is aborted.
int farm_wait(lfm_ctx* ctx, const unsigned* seq_word, unsigned seq, int64_t count, double* recv) {
  hipError_t e;
  // one bounded wait for the whole chain (kernel, collective, publish): the sequence word — a
  // tight spin for the first 2 ms (a round takes tens of microseconds), then the stream is
  // polled between backed-off checks, so a fault surfaces instead of running out the bound
  const double end = mono_s() + rccl_timeout_s(ctx);
  const Backoff bo;
  const auto t_spin = std::chrono::steady_clock::now() + std::chrono::milliseconds(2);
  // published: the sequence word AND every slot (each marked RESULT_PENDING before the round;
  // no reliance on the order in which the slots' and the word's writes reach host memory)
  auto published = [&] {
    return __atomic_load_n(seq_word, __ATOMIC_ACQUIRE) == seq && all_landed(ctx->farm_pub, count);
  };
  while (!published() && std::chrono::steady_clock::now() < t_spin) __builtin_ia32_pause();
  while (!published()) {
    e = hipStreamQuery(ctx->stream);
    if (e != hipSuccess && e != hipErrorNotReady) {
      rccl_drop(ctx);
      return hip_fail(ctx, e, "farm round");
    }
    if (e == hipSuccess && !published()) {
      rccl_drop(ctx);
      return set_err(ctx, LFM_E_HIP, "farm round: the stream drained without publishing");
    }
    const double now = mono_s();
    if (now > end) {
      char waited[64];
      std::snprintf(waited, sizeof(waited), " after %.2f s", now - bo.t0);
      rccl_drop(ctx);
      return set_err(ctx, LFM_E_RCCL, std::string("farm round: timed out") + waited +
                                          " (a peer rank did not arrive)");
    }
    bo.pause();
  }
  std::memcpy(recv, ctx->farm_pub, (size_t)count * 8);
  return LFM_OK;
}

// Enqueue the all-gather of `slots` doubles per rank (send -> recv, device) and the publish of
// recv to the pinned host buffer, then wait (bounded) for the round's sequence word; on any error
// or timeout the communicator is aborted (LFM_E_RCCL / LFM_E_HIP) and nothing is copied out.
int farm_gather_publish(lfm_ctx* ctx, int64_t slots, double* recv) {
  double* dsend = ctx->farm_buf;
  double* drecv = ctx->farm_buf + slots;
  const int64_t count = slots * ctx->nranks;
  unsigned* seq_word = reinterpret_cast<unsigned*>(ctx->farm_pub + count);
  int r = farm_allgather(ctx, dsend, drecv, slots);
  if (r) {
    rccl_drop(ctx);
    return r;
  }
  const unsigned seq = ++ctx->farm_seq;
  mark_pending(ctx->farm_pub, count);
  hipLaunchKernelGGL(farm_publish_kernel, dim3(1), dim3(64), 0, ctx->stream, drecv, count,
                     ctx->farm_pub.p, seq_word, seq);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    rccl_drop(ctx);
    return hip_fail(ctx, e, "farm publish");
  }
  return farm_wait(ctx, seq_word, seq, count, recv);
}

// The round's publish value when it is replayed from the captured graph (a graph's kernel
// arguments are fixed): the host clears the word before each replay. The enqueued path counts
// from 1 and never reaches it.
constexpr unsigned FARM_GRAPH_SEQ = 0xFFFFFFFFu;

// Capture one device-side round — the padding memset (slots > nprob), the batch's MLL kernel
// reading its hyperparameters from the batch's pinned buffer, ncclAllGather, the publish kernel —
// as a graph, so a round costs one graph launch instead of three enqueues and RCCL's host-side
// enqueue of the collective (which left the GPU idle between the kernel and the collective).
// Returns LFM_OK with ctx->farm_exec set, or non-zero when capture is not possible (the caller
// then enqueues; the graph stays off for this context).
int farm_graph_build(lfm_ctx* ctx, lfm_batch* batch, int negative, int64_t slots) {
  farm_graph_reset(ctx);
  small_batch_attrs();
  const int64_t np = batch->nprob;
  double* dsend = ctx->farm_buf;
  double* drecv = ctx->farm_buf + slots;
  const int64_t count = slots * ctx->nranks;
  unsigned* seq_word = reinterpret_cast<unsigned*>(ctx->farm_pub + count);
  hipError_t e = hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeRelaxed);
  if (e != hipSuccess) return hip_fail(ctx, e, "farm graph: begin capture");
  int r = LFM_OK;
  if (slots > np)
    e = hipMemsetAsync(dsend + np, 0xFF, (size_t)(slots - np) * 8, ctx->stream);
  if (e == hipSuccess)
    r = launch_small_batch(ctx, batch->dprobs, (int)np, plan_small_mll(batch->dims), negative,
                           dsend, batch_words(batch));
  else
    r = hip_fail(ctx, e, "farm graph: padding");
  if (!r) r = farm_allgather(ctx, dsend, drecv, slots);  // the test instrument is captured too
  if (!r) {
    hipLaunchKernelGGL(farm_publish_kernel, dim3(1), dim3(64), 0, ctx->stream, drecv, count,
                       ctx->farm_pub.p, seq_word, FARM_GRAPH_SEQ);
    r = hip_fail(ctx, hipGetLastError(), "farm graph: publish");
  }
  hipGraph_t graph = nullptr;
  e = hipStreamEndCapture(ctx->stream, &graph);
  if (!r && e != hipSuccess) r = hip_fail(ctx, e, "farm graph: end capture");
  if (!r) {
    e = hipGraphInstantiate(&ctx->farm_exec, graph, nullptr, nullptr, 0);
    if (e != hipSuccess) {
      ctx->farm_exec = nullptr;
      r = hip_fail(ctx, e, "farm graph: instantiate");
    }
  }
  if (graph) hipGraphDestroy(graph);
  (void)hipGetLastError();
  if (r) {
    farm_graph_reset(ctx);
    return r;
  }
  ctx->farm_exec_batch = batch->id;
  ctx->farm_exec_slots = slots;
  ctx->farm_exec_neg = negative;
  ctx->farm_exec_gen = ctx->comm_gen;
  return LFM_OK;
}
}  // namespace

extern "C" {

int lfm_farm_unique_id(lfm_ctx* ctx, unsigned char id[128]) {
  if (!ctx || !id) return LFM_E_ARG;
  int r = rccl_load(ctx);
  if (r) return r;
  DeviceGuard g(ctx->device);
  ncclUniqueId u;
  r = rccl_fail(ctx, g_rccl.getUniqueId(&u), "ncclGetUniqueId");
  if (r) return r;
  std::memcpy(id, u.internal, 128);
  return LFM_OK;
}

int lfm_farm_init(lfm_ctx* ctx, const unsigned char id[128], int nranks, int rank) {
  if (!ctx || !id || nranks < 1 || rank < 0 || rank >= nranks) return LFM_E_ARG;
  int r = rccl_load(ctx);
  if (r) return r;
  DeviceGuard g(ctx->device);
  if (ctx->comm) lfm_farm_destroy(ctx);
  ncclUniqueId u;
  std::memcpy(u.internal, id, 128);
  ncclComm_t comm = nullptr;
  bool nb = false;
  if (g_rccl.commInitRankConfig && g_rccl.commGetAsyncError && g_rccl.commAbort) {
    // non-blocking communicator: the init (and every later call) is polled against a deadline
    ncclConfig_t cfg = NCCL_CONFIG_INITIALIZER;
    cfg.blocking = 0;
    const ncclResult_t q = g_rccl.commInitRankConfig(&comm, nranks, u, rank, &cfg);
    if (q == ncclSuccess || q == ncclInProgress) {
      r = rccl_poll(ctx, comm, "ncclCommInitRankConfig");
      if (r) {
        g_rccl.commAbort(comm);
        return r;
      }
      nb = true;
    } else if (q != ncclInvalidArgument) {
      return rccl_fail(ctx, q, "ncclCommInitRankConfig");
    } else {
      comm = nullptr;  // a library that rejects this config layout: blocking init below
    }
  }
  if (!nb) {
    r = rccl_fail(ctx, g_rccl.commInitRank(&comm, nranks, u, rank), "ncclCommInitRank");
    if (r) return r;
  }
  ctx->comm = comm;
  ctx->comm_nb = nb;
  ctx->nranks = nranks;
  ctx->rank = rank;
  ++ctx->comm_gen;
  return LFM_OK;
}

int lfm_farm_batch_mll_f64(lfm_ctx* ctx, lfm_batch* batch, const double* hyp, int negative,
                           int64_t slots, double* recv, int* status) {
  if (!ctx) return LFM_E_ARG;
  if (!batch || !hyp || !recv || slots < batch->nprob || slots < 1)
    return set_err(ctx, LFM_E_ARG, "bad farm round arguments (slots >= nprob >= 1)");
  if (batch->device != ctx->device) return set_err(ctx, LFM_E_ARG, "batch of another device");
  if (!ctx->comm) return set_err(ctx, LFM_E_STATE, "farm not initialised");
  DeviceGuard g(ctx->device);
  int r = farm_drain_stale(ctx);
  if (!r) r = farm_buffers(ctx, (size_t)slots);
  if (r) return r;
  // replayed from the captured graph (not while profiling: its events want the enqueued launches)
  if (ctx->knobs.farm_graph_on && !ctx->prof) {
    if (!ctx->farm_exec || ctx->farm_exec_batch != batch->id || ctx->farm_exec_slots != slots ||
        ctx->farm_exec_neg != negative || ctx->farm_exec_gen != ctx->comm_gen) {
      // capture not possible here: enqueue from now on (an error of the collective itself
      // surfaces again on the enqueued path below)
      if (farm_graph_build(ctx, batch, negative, slots)) ctx->knobs.farm_graph_on = false;
    }
    if (ctx->farm_exec) {
      const int64_t count = slots * ctx->nranks;
      std::memcpy(batch->hbuf, hyp, (size_t)batch->nhyp * 8);
      batch_reset(batch);
      unsigned* seq_word = reinterpret_cast<unsigned*>(ctx->farm_pub + count);
      mark_pending(ctx->farm_pub, count);
      __atomic_store_n(seq_word, 0u, __ATOMIC_RELEASE);
      hipError_t e = hipGraphLaunch(ctx->farm_exec, ctx->stream);
      if (e != hipSuccess) {
        rccl_drop(ctx);
        return hip_fail(ctx, e, "farm graph launch");
      }
      hipEventRecord(batch->done, ctx->stream);
      r = farm_wait(ctx, seq_word, FARM_GRAPH_SEQ, count, recv);
      if (r) return r;
      return batch_status(ctx, batch_words(batch), batch->nprob, status);
    }
  }
  // this rank's padding slots: NaN (all-ones bytes), then the kernel writes its nprob slots
  if (slots > batch->nprob) {
    const hipError_t e = hipMemsetAsync(ctx->farm_buf + batch->nprob, 0xFF,
                                        (size_t)(slots - batch->nprob) * 8, ctx->stream);
    if (e != hipSuccess) return hip_fail(ctx, e, "farm round: padding slots");
  }
  r = batch_launch(ctx, batch, hyp, negative, ctx->farm_buf);
  if (r) return r;
  r = farm_gather_publish(ctx, slots, recv);
  if (r) return r;
  // the statuses landed before the kernel retired, and the kernel before the collective
  return batch_status(ctx, batch_words(batch), batch->nprob, status);
}

int lfm_farm_allgather_f64(lfm_ctx* ctx, const double* send, int64_t count, double* recv) {
  if (!ctx || !send || !recv || count < 1) return LFM_E_ARG;
  if (!ctx->comm) return set_err(ctx, LFM_E_STATE, "farm not initialised");
  DeviceGuard g(ctx->device);
  int rs = farm_drain_stale(ctx);
  if (rs) return rs;
  const size_t in = (size_t)count * 8, out = in * ctx->nranks;
  int r = farm_device_buffer(ctx, in + out);
  if (r) return r;
  // host side through a pinned buffer of the farm's own: every copy is truly asynchronous (a
  // copy into pageable memory would block past the deadline below), and a copy a timed-out call
  // leaves queued can only ever write into this buffer — never the caller's, never the staging
  // other calls use
  r = ctx->farm_h.reserve(ctx, in + out, hipHostMallocDefault, "farm staging buffer");
  if (r) return r;
  double* hsend = ctx->farm_h;
  double* hrecv = ctx->farm_h + count;
  double* dsend = ctx->farm_buf;
  double* drecv = ctx->farm_buf + count;
  std::memcpy(hsend, send, in);
  hipError_t e = hipMemcpyAsync(dsend, hsend, in, hipMemcpyHostToDevice, ctx->stream);
  if (e != hipSuccess) return hip_fail(ctx, e, "farm upload");
  r = farm_allgather(ctx, dsend, drecv, count);
  if (!r) {
    e = hipMemcpyAsync(hrecv, drecv, out, hipMemcpyDeviceToHost, ctx->stream);
    if (e != hipSuccess) r = hip_fail(ctx, e, "farm download");
  }
  // one bounded wait for the collective and the copy behind it (the latency-bound exchange has
  // a single synchronisation point); a blocking communicator waits unbounded, as RCCL would
  if (!r) r = ctx->comm_nb ? rccl_stream_wait(ctx, "ncclAllGather") : finish(ctx);
  if (r) {
    rccl_drop(ctx);
    return r;
  }
  std::memcpy(recv, hrecv, out);
  return LFM_OK;
}

int lfm_farm_destroy(lfm_ctx* ctx) {
  if (!ctx) return LFM_E_ARG;
  farm_graph_reset(ctx);
  if (ctx->farm_exec_old && hipStreamQuery(ctx->stream) == hipSuccess) {
    hipGraphExecDestroy(ctx->farm_exec_old);
    ctx->farm_exec_old = nullptr;
  }
  if (ctx->comm && g_rccl.commDestroy) g_rccl.commDestroy((ncclComm_t)ctx->comm);
  ctx->comm = nullptr;
  ctx->nranks = 0;
  ctx->rank = -1;
  return LFM_OK;
}

}  // extern "C"
