// Step programs: the native step driver of the training loop (src/train_fibinet.py:113-123).
//
// One training step is ~25 launches of this library's C-ABI entry points on two streams with a
// few cross-stream edges.  Issued from Python (ctypes conversion + the trainer's sequencing) that
// costs ~0.4 ms of host time per step at C3 -- as much as the GPU work.  hipGraph replay avoids
// the host cost but adds its own per-edge cost for multi-stream graphs.  A step program is the
// third way: the host records the step's calls ONCE (entry point, its arguments, the stream
// edges) while running it, and replays them natively: the same launches on the same streams in
// the same order, so a replay is bit-identical to the eager step it was recorded from.
//
// Replay calls each recorded entry point through a packed-argument thunk that the compiler makes
// from the prototype include/fibinet.h declares (template Thunk below; one table line per
// recordable entry point): the thunk takes the recorded arguments as two arrays -- integer-class
// values (pointers, int, long long, size_t) as 64-bit words, float / double values as doubles (a
// float in the low 32 bits of its double) -- and makes an ordinary, well-typed call of the entry
// point.  A recording names the entry point; its argument counts are checked against the thunk's.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <type_traits>
#include <utility>
#include <vector>

#include "fibinet.h"

void fbn_set_error(const char* msg);

namespace {

constexpr int kMaxInt = 48;
constexpr int kMaxFlt = 8;

typedef uint64_t U;
typedef int (*ThunkFn)(const U* i, const double* f);

struct PlanThunk {
  const char* name;
  ThunkFn fn;
  int ni, nf;
};

// a float argument: the low 32 bits of its double slot (the recorder's encoding)
inline float plan_f32(double d) {
  uint64_t b;
  memcpy(&b, &d, sizeof(b));
  const uint32_t lo = (uint32_t)b;
  float x;
  memcpy(&x, &lo, sizeof(x));
  return x;
}

// The thunk of entry point Fn, from its prototype int (A...): argument k is slot(k) of its class's
// array, where slot(k) counts the earlier arguments of the same class.
template <auto Fn>
struct Thunk;
template <class... A, int (*Fn)(A...)>
struct Thunk<Fn> {
  template <class T>
  static constexpr bool is_flt = std::is_floating_point<T>::value;
  static constexpr int nf = (0 + ... + int(is_flt<A>));
  static constexpr int ni = int(sizeof...(A)) - nf;
  static_assert(ni <= kMaxInt && nf <= kMaxFlt, "an Op cannot hold this entry point's arguments");

  static constexpr int slot(int k) {
    constexpr bool flt[] = {is_flt<A>..., false};
    int n = 0;
    for (int j = 0; j < k; ++j) n += flt[j] == flt[k];
    return n;
  }
  template <class T, int K>
  static T arg(const U* i, const double* f) {
    if constexpr (std::is_same<T, float>::value) return plan_f32(f[K]);
    else if constexpr (std::is_same<T, double>::value) return f[K];
    else if constexpr (std::is_pointer<T>::value) return reinterpret_cast<T>(static_cast<uintptr_t>(i[K]));
    else return static_cast<T>(i[K]);
  }
  template <size_t... K>
  static int call(const U* i, const double* f, std::index_sequence<K...>) {
    (void)i, (void)f;
    return Fn(arg<A, slot(K)>(i, f)...);
  }
  static int run(const U* i, const double* f) { return call(i, f, std::index_sequence_for<A...>{}); }
};

// fbn_adam_catchup's arguments 13..15 (wd, beta2, eps) are floats between integers
static_assert(Thunk<fbn_adam_catchup>::ni == 20 && Thunk<fbn_adam_catchup>::nf == 3, "argument classes");
static_assert(Thunk<fbn_adam_catchup>::slot(12) == 12 && Thunk<fbn_adam_catchup>::slot(13) == 0 &&
                  Thunk<fbn_adam_catchup>::slot(15) == 2 && Thunk<fbn_adam_catchup>::slot(16) == 13,
              "a slot counts the earlier arguments of its own class only");
static_assert(Thunk<fbn_probe_disarm>::ni == 0 && Thunk<fbn_probe_disarm>::nf == 0, "no arguments");

// Every int-returning entry point a step program may replay: all but the program machinery itself
// (fbn_plan_*) and the communicator's setup and watchdog calls.  Sorted by name (find_thunk).
#define FBN_THUNK(fn) {#fn, Thunk<fn>::run, Thunk<fn>::ni, Thunk<fn>::nf}
constexpr PlanThunk kPlanThunks[] = {
    FBN_THUNK(fbn_adam_catchup),
    FBN_THUNK(fbn_adam_claim_catchup),
    FBN_THUNK(fbn_adam_claim_catchup_conv),
    FBN_THUNK(fbn_adam_commit),
    FBN_THUNK(fbn_adam_dense),
    FBN_THUNK(fbn_adam_flush),
    FBN_THUNK(fbn_adam_owner_claim_catchup),
    FBN_THUNK(fbn_adam_prefetch),
    FBN_THUNK(fbn_adam_prefetch_binned),
    FBN_THUNK(fbn_adam_prefetch_rows),
    FBN_THUNK(fbn_adam_selftest),
    FBN_THUNK(fbn_adam_step_tail),
    FBN_THUNK(fbn_adam_table),
    FBN_THUNK(fbn_adam_touched),
    FBN_THUNK(fbn_auc_place),
    FBN_THUNK(fbn_bilinear_bwd),
    FBN_THUNK(fbn_bilinear_fields_bwd),
    FBN_THUNK(fbn_bilinear_fields_bwd_supported),
    FBN_THUNK(fbn_bilinear_fwd),
    FBN_THUNK(fbn_bilinear_supported),
    FBN_THUNK(fbn_bn_act_fwd),
    FBN_THUNK(fbn_bn_act_fwd_img),
    FBN_THUNK(fbn_bn_act_head_fwd),
    FBN_THUNK(fbn_bn_act_head_fwd_w),
    FBN_THUNK(fbn_bn_bwd),
    FBN_THUNK(fbn_bn_bwd_apply),
    FBN_THUNK(fbn_bn_bwd_chunks),
    FBN_THUNK(fbn_bn_bwd_fused),
    FBN_THUNK(fbn_bn_bwd_fused_img),
    FBN_THUNK(fbn_bn_bwd_reduce),
    FBN_THUNK(fbn_bn_eval_params),
    FBN_THUNK(fbn_bn_finalize),
    FBN_THUNK(fbn_bn_mean),
    FBN_THUNK(fbn_bn_moments_finalize),
    FBN_THUNK(fbn_bn_stats),
    FBN_THUNK(fbn_bn_stats_pass),
    FBN_THUNK(fbn_bn_tile_finalize),
    FBN_THUNK(fbn_bn_tile_moments),
    FBN_THUNK(fbn_bn_tile_stats),
    FBN_THUNK(fbn_calib_reduce),
    FBN_THUNK(fbn_claim_rows),
    FBN_THUNK(fbn_clip_coef),
    FBN_THUNK(fbn_collate),
    FBN_THUNK(fbn_collate_f32),
    FBN_THUNK(fbn_collate_zero_if),
    FBN_THUNK(fbn_colsum),
    FBN_THUNK(fbn_colsum_partial),
    FBN_THUNK(fbn_comm_allgather),
    FBN_THUNK(fbn_comm_allreduce),
    FBN_THUNK(fbn_comm_alltoall),
    FBN_THUNK(fbn_comm_alltoall_peers),
    FBN_THUNK(fbn_comm_alltoallv),
    FBN_THUNK(fbn_comm_heartbeat),
    FBN_THUNK(fbn_comm_id_bytes),
    FBN_THUNK(fbn_compact_routes),
    FBN_THUNK(fbn_convert_bf16),
    FBN_THUNK(fbn_copy_jobs),
    FBN_THUNK(fbn_delong_reduce),
    FBN_THUNK(fbn_device_ok),
    FBN_THUNK(fbn_digest_u64),
    FBN_THUNK(fbn_eval_pack),
    FBN_THUNK(fbn_eval_pack_groups),
    FBN_THUNK(fbn_eval_reduce),
    FBN_THUNK(fbn_fields_bwd),
    FBN_THUNK(fbn_fields_bwd_grid),
    FBN_THUNK(fbn_fields_bwd_img),
    FBN_THUNK(fbn_fields_bwd_partials_size),
    FBN_THUNK(fbn_fields_bwd_slot),
    FBN_THUNK(fbn_fields_fwd),
    FBN_THUNK(fbn_fields_fwd_hot),
    FBN_THUNK(fbn_gauc_reduce),
    FBN_THUNK(fbn_gemm),
    FBN_THUNK(fbn_gemm_bf16out),
    FBN_THUNK(fbn_gemm_bn_bwd_part),
    FBN_THUNK(fbn_gemm_bn_bwd_part_supported),
    FBN_THUNK(fbn_gemm_s3),
    FBN_THUNK(fbn_gemm_slabs),
    FBN_THUNK(fbn_gemm_slabs_group),
    FBN_THUNK(fbn_gemm_slabs_group_split),
    FBN_THUNK(fbn_gemm_slabs_split),
    FBN_THUNK(fbn_gemm_split),
    FBN_THUNK(fbn_head_fwd),
    FBN_THUNK(fbn_head_fwd_w),
    FBN_THUNK(fbn_hot_rows),
    FBN_THUNK(fbn_isotonic_apply),
    FBN_THUNK(fbn_isotonic_fit),
    FBN_THUNK(fbn_knn_normalize),
    FBN_THUNK(fbn_knn_query_pool),
    FBN_THUNK(fbn_knn_scores),
    FBN_THUNK(fbn_list_ild),
    FBN_THUNK(fbn_mmr_select),
    FBN_THUNK(fbn_owner_claim),
    FBN_THUNK(fbn_owner_fold),
    FBN_THUNK(fbn_owner_gather),
    FBN_THUNK(fbn_owner_gather_self),
    FBN_THUNK(fbn_pack_extras),
    FBN_THUNK(fbn_pad_routes),
    FBN_THUNK(fbn_pairs_bwd),
    FBN_THUNK(fbn_pairs_bwd_img),
    FBN_THUNK(fbn_pairs_fwd),
    FBN_THUNK(fbn_pairs_fwd_img),
    FBN_THUNK(fbn_probe_arm),
    FBN_THUNK(fbn_probe_disarm),
    FBN_THUNK(fbn_rank_hist),
    FBN_THUNK(fbn_rec_fields),
    FBN_THUNK(fbn_rec_fields_list),
    FBN_THUNK(fbn_rec_hist_pool),
    FBN_THUNK(fbn_rec_item_cache),
    FBN_THUNK(fbn_rec_rank),
    FBN_THUNK(fbn_rec_rank_list),
    FBN_THUNK(fbn_rec_topk),
    FBN_THUNK(fbn_rec_topk_list),
    FBN_THUNK(fbn_ring_slot),
    FBN_THUNK(fbn_route),
    FBN_THUNK(fbn_route_fc),
    FBN_THUNK(fbn_route_fc_status),
    FBN_THUNK(fbn_row_chunks),
    FBN_THUNK(fbn_sigmoid_bwd),
    FBN_THUNK(fbn_sort_u64),
    FBN_THUNK(fbn_sparse_fixup),
    FBN_THUNK(fbn_sparse_fixup_dup),
    FBN_THUNK(fbn_sparse_fold_fx),
    FBN_THUNK(fbn_step_end),
    FBN_THUNK(fbn_sum_jobs),
    FBN_THUNK(fbn_sum_jobs2),
    FBN_THUNK(fbn_sum_jobs_sq),
    FBN_THUNK(fbn_sum_slices),
    FBN_THUNK(fbn_sumsq),
    FBN_THUNK(fbn_sumsq_flagged),
    FBN_THUNK(fbn_sumsq_sparse),
    FBN_THUNK(fbn_sumsq_sparse_norms),
    FBN_THUNK(fbn_unpack_extras),
    FBN_THUNK(fbn_unpack_sumsq),
    FBN_THUNK(fbn_version),
    FBN_THUNK(fbn_widen_bf16),
};
#undef FBN_THUNK

constexpr bool thunks_sorted() {
  for (size_t k = 1; k < sizeof(kPlanThunks) / sizeof(kPlanThunks[0]); ++k) {
    const char *a = kPlanThunks[k - 1].name, *b = kPlanThunks[k].name;
    while (*a && *a == *b) ++a, ++b;
    if ((unsigned char)*a >= (unsigned char)*b) return false;
  }
  return true;
}
static_assert(thunks_sorted(), "find_thunk searches kPlanThunks by name");

const PlanThunk* find_thunk(const char* name) {
  size_t lo = 0, hi = sizeof(kPlanThunks) / sizeof(kPlanThunks[0]);
  while (lo < hi) {
    const size_t mid = (lo + hi) / 2;
    const int c = strcmp(kPlanThunks[mid].name, name);
    if (c == 0) return &kPlanThunks[mid];
    if (c < 0) lo = mid + 1;
    else hi = mid;
  }
  return nullptr;
}

enum OpKind { kCall = 0, kRecord = 1, kWait = 2 };

struct Op {
  int kind;
  int slot;                // kRecord / kWait: event slot
  ThunkFn fn;              // kCall
  hipStream_t stream;      // kRecord / kWait
  U i[kMaxInt];
  double f[kMaxFlt];
};

struct Plan {
  int device;
  std::vector<Op> ops;
  std::vector<hipEvent_t> events;
};

int call_op(const Op& o) { return o.fn(o.i, o.f); }

// The program's events only order work between streams of one device, so their release need not be
// system scope (the default: an L2 writeback + invalidate at every record, ~6 us of idle on the
// recording stream before its next kernel).
constexpr unsigned kEventFlags = hipEventDisableTiming | hipEventDisableSystemFence;

int ensure_event(Plan* p, int slot) {
  while ((int)p->events.size() <= slot) {
    hipEvent_t e;
    if (hipEventCreateWithFlags(&e, kEventFlags) != hipSuccess) {
      fbn_set_error("fbn_plan: hipEventCreateWithFlags failed");
      return 2;
    }
    p->events.push_back(e);
  }
  return 0;
}

}  // namespace

extern "C" int fbn_plan_create(void** out) {
  if (!out) {
    fbn_set_error("fbn_plan_create: null out");
    return 1;
  }
  Plan* p = new Plan();
  if (hipGetDevice(&p->device) != hipSuccess) p->device = 0;
  *out = p;
  return 0;
}

extern "C" int fbn_plan_destroy(void* plan) {
  Plan* p = static_cast<Plan*>(plan);
  if (!p) return 0;
  for (hipEvent_t e : p->events) (void)hipEventDestroy(e);
  delete p;
  return 0;
}

extern "C" int fbn_plan_size(void* plan) { return plan ? (int)static_cast<Plan*>(plan)->ops.size() : 0; }

extern "C" int fbn_plan_add_call(void* plan, const char* name, const unsigned long long* iargs, int ni,
                                 const double* fargs, int nf) {
  Plan* p = static_cast<Plan*>(plan);
  if (!p || !name || ni < 0 || nf < 0 || ni > kMaxInt || nf > kMaxFlt || (ni && !iargs) || (nf && !fargs)) {
    fbn_set_error("fbn_plan_add_call: bad arguments");
    return 1;
  }
  const PlanThunk* t = find_thunk(name);
  if (!t) {
    fbn_set_error("fbn_plan_add_call: not a recordable entry point of fibinet.h");
    return 1;
  }
  if (t->ni != ni || t->nf != nf) {
    fbn_set_error("fbn_plan_add_call: argument counts differ from the entry point's prototype");
    return 1;
  }
  Op o;
  memset(&o, 0, sizeof(o));
  o.kind = kCall;
  o.fn = t->fn;
  for (int k = 0; k < ni; ++k) o.i[k] = iargs[k];
  for (int k = 0; k < nf; ++k) o.f[k] = fargs[k];
  p->ops.push_back(o);
  return 0;
}

// stream edge, first half: record event `slot` on `stream` (hipEventRecord)
extern "C" int fbn_plan_add_record(void* plan, int slot, void* stream) {
  Plan* p = static_cast<Plan*>(plan);
  if (!p || slot < 0) {
    fbn_set_error("fbn_plan_add_record: bad arguments");
    return 1;
  }
  if (int rc = ensure_event(p, slot)) return rc;
  Op o;
  memset(&o, 0, sizeof(o));
  o.kind = kRecord;
  o.slot = slot;
  o.stream = static_cast<hipStream_t>(stream);
  p->ops.push_back(o);
  return 0;
}

// stream edge, second half: `stream` waits for event `slot` (hipStreamWaitEvent)
extern "C" int fbn_plan_add_wait(void* plan, void* stream, int slot) {
  Plan* p = static_cast<Plan*>(plan);
  if (!p || slot < 0) {
    fbn_set_error("fbn_plan_add_wait: bad arguments");
    return 1;
  }
  if (int rc = ensure_event(p, slot)) return rc;
  Op o;
  memset(&o, 0, sizeof(o));
  o.kind = kWait;
  o.slot = slot;
  o.stream = static_cast<hipStream_t>(stream);
  p->ops.push_back(o);
  return 0;
}

// Host wait for the program's event `slot` as its last replay (or the recording run) left it -- the
// sharded step's host check of the routed-ahead overflow flag waits for the routing this way.
extern "C" int fbn_plan_event_sync(void* plan, int slot) {
  Plan* p = static_cast<Plan*>(plan);
  if (!p || slot < 0 || slot >= (int)p->events.size()) {
    fbn_set_error("fbn_plan_event_sync: bad arguments");
    return 1;
  }
  if (hipEventSynchronize(p->events[slot]) != hipSuccess) {
    fbn_set_error("fbn_plan_event_sync: hipEventSynchronize failed");
    return 2;
  }
  return 0;
}

// Replay every recorded op in order.  Returns 0, or the failing entry point's code (its
// message stays in fbn_last_error) with *failed = the op index.
extern "C" int fbn_plan_run(void* plan, int* failed) {
  Plan* p = static_cast<Plan*>(plan);
  if (!p) {
    fbn_set_error("fbn_plan_run: null plan");
    return 1;
  }
  int n = (int)p->ops.size();
  for (int k = 0; k < n; ++k) {
    const Op& o = p->ops[k];
    int rc = 0;
    if (o.kind == kCall) {
      rc = call_op(o);
    } else if (o.kind == kRecord) {
      if (hipEventRecord(p->events[o.slot], o.stream) != hipSuccess) {
        fbn_set_error("fbn_plan_run: hipEventRecord failed");
        rc = 2;
      }
    } else {
      if (hipStreamWaitEvent(o.stream, p->events[o.slot], 0) != hipSuccess) {
        fbn_set_error("fbn_plan_run: hipStreamWaitEvent failed");
        rc = 2;
      }
    }
    if (rc) {
      if (failed) *failed = k;
      return rc;
    }
  }
  return 0;
}
