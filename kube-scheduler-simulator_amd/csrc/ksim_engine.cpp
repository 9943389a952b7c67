// ksim_engine.cpp — host runtime behind the C ABI (include/ksim_engine.h).
//
// Owns the HBM-resident snapshot (SoA node columns, vocabularies), the pod
// queue, the per-cycle scratch and one HIP stream.  Batch runs are split into
// maximal runs of pods the speculative batch path can take (P100 and no
// node-varying normalized score) and runs that need the per-pod path; each
// path is a captured hipGraph replayed until the run's cursor is consumed.
// Every input is validated on the host before any kernel sees it (a bad index
// must never reach the device), copied during the call, never retained.
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <tuple>
#include <unordered_map>
#include <type_traits>
#include <vector>

#include "ksim_host.h"

using namespace ksim_host;

namespace {

constexpr int kGraphCycles = 128;      // per-pod cycles per captured graph

// RCCL, resolved at run time: the process may already hold torch's librccl
// (RTLD_NOLOAD finds it first, so both share one RCCL and one HIP runtime).
struct Rccl {
  bool ok = false;
  decltype(&ncclGetUniqueId) get_unique_id = nullptr;
  decltype(&ncclCommInitRank) comm_init_rank = nullptr;
  decltype(&ncclCommDestroy) comm_destroy = nullptr;
  decltype(&ncclAllGather) all_gather = nullptr;
  decltype(&ncclAllReduce) all_reduce = nullptr;
  decltype(&ncclGetErrorString) error_string = nullptr;
};

const Rccl& rccl() {
  static Rccl r = [] {
    Rccl x;
    void* lib = nullptr;
    for (const char* name : {"librccl.so", "librccl.so.1"})
      if (!lib) lib = dlopen(name, RTLD_NOW | RTLD_NOLOAD);
    for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"})
      if (!lib) lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
    if (!lib) return x;
    x.get_unique_id = (decltype(x.get_unique_id))dlsym(lib, "ncclGetUniqueId");
    x.comm_init_rank = (decltype(x.comm_init_rank))dlsym(lib, "ncclCommInitRank");
    x.comm_destroy = (decltype(x.comm_destroy))dlsym(lib, "ncclCommDestroy");
    x.all_gather = (decltype(x.all_gather))dlsym(lib, "ncclAllGather");
    x.all_reduce = (decltype(x.all_reduce))dlsym(lib, "ncclAllReduce");
    x.error_string = (decltype(x.error_string))dlsym(lib, "ncclGetErrorString");
    x.ok = x.get_unique_id && x.comm_init_rank && x.comm_destroy && x.all_gather && x.all_reduce && x.error_string;
    return x;
  }();
  return r;
}
constexpr int kGraphBatches = 16;      // speculative batches per captured graph

}  // namespace

namespace ksim_host {

int set_err(ksim_handle* h, int code, const std::string& msg) {
  if (h) h->err = msg;
  return code;
}

int hip_fail(ksim_handle* h, hipError_t e, const char* what) {
  int code = (e == hipErrorOutOfMemory) ? KSIM_E_OOM : KSIM_E_DEVICE;
  return set_err(h, code, std::string(what) + ": " + hipGetErrorString(e));
}

// Blocking copies on the handle's own non-blocking stream.  A hipMemcpy on the
// legacy stream is refused while another host thread captures a graph (several
// engines in one process: bench config 5's concurrent sweep), and stream order
// is the order the engine relies on anyway.
hipError_t hcopy(ksim_handle* h, void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
  const hipError_t e = hipMemcpyAsync(dst, src, bytes, kind, h->stream);
  return e != hipSuccess ? e : hipStreamSynchronize(h->stream);
}

static hipError_t hzero(ksim_handle* h, void* dst, size_t bytes) {
  const hipError_t e = hipMemsetAsync(dst, 0, bytes, h->stream);
  return e != hipSuccess ? e : hipStreamSynchronize(h->stream);
}

}  // namespace ksim_host

// ---- ksim_mem.h: the calls that allocate ---------------------------------------
// Allocate + copy (src may be null: zero-filled).
int DevPool::upload(ksim_handle* h, const void* src, size_t bytes, void** out) {
  void* p = nullptr;
  size_t alloc = bytes ? bytes : 16;
  hipError_t e = hipMalloc(&p, alloc);
  if (e != hipSuccess) return hip_fail(h, e, "hipMalloc");
  v_.push_back({p, alloc});
  if (src && bytes) {
    e = hipMemcpyAsync(p, src, bytes, hipMemcpyHostToDevice, h->stream);
  } else {
    e = hipMemsetAsync(p, 0, alloc, h->stream);
  }
  if (e != hipSuccess) return hip_fail(h, e, "upload copy");
  *out = p;
  return KSIM_OK;
}

// The reserve rule is ksim_mem.h's (Idle); a failed allocation leaves the buffer empty.
int DevGrow::reserve(ksim_handle* h, size_t bytes, Idle idle) {
  if (bytes <= cap) return KSIM_OK;
  if (idle == Idle::kSync) HIPCHK(h, hipStreamSynchronize(h->stream));
  if (p) (void)hipFree(p);
  p = nullptr;
  cap = 0;
  const size_t want = floor_ ? std::max(bytes * 2, floor_) : std::max<size_t>(bytes, 16);
  const hipError_t e = hipMalloc(&p, want);
  if (e != hipSuccess) {
    p = nullptr;
    return hip_fail(h, e, what_);
  }
  cap = want;
  return KSIM_OK;
}

int PinGrow::reserve(ksim_handle* h, size_t bytes, Idle idle) {
  if (bytes <= cap) return KSIM_OK;
  if (idle == Idle::kSync) HIPCHK(h, hipStreamSynchronize(h->stream));
  if (p) (void)hipHostFree(p);
  p = d = nullptr;
  cap = 0;
  const size_t want = floor_ ? std::max(bytes * 2, floor_) : std::max<size_t>(bytes, 16);
  hipError_t e = hipHostMalloc(&p, want, flags_);
  if (e != hipSuccess) {
    p = nullptr;
    return hip_fail(h, e, what_);
  }
  if ((flags_ & hipHostMallocMapped) && (e = hipHostGetDevicePointer(&d, p, 0)) != hipSuccess)
    return hip_fail(h, e, "hipHostGetDevicePointer");   // cap stays 0: the next reserve starts over
  cap = want;
  return KSIM_OK;
}

namespace {

// The shard-group graphs a leader holds (group_graph).
void drop_group_graphs(ksim_handle* h) {
  for (auto& kv : h->sg_graphs) (void)hipGraphExecDestroy(kv.second);
  h->sg_graphs.clear();
}

// The handle's own graphs whose key `pred` picks (ksim_host.h GraphKey): the
// one place that destroys them, whatever the scope.
template <class P>
void drop_graphs_if(ksim_handle* h, P&& pred) {
  for (auto it = h->graphs.begin(); it != h->graphs.end();)
    it = pred(it->first) ? ((void)hipGraphExecDestroy(it->second), h->graphs.erase(it)) : std::next(it);
}

constexpr auto is_lazy = [](const GraphKey& k) { return k.kind == GraphKind::kLazy; };
constexpr auto is_table = [](const GraphKey& k) { return k.kind == GraphKind::kLazy && k.arg[1] > 0; };

// The per-pod cycle graphs (their kernels take the profile by value), and the
// group graphs, which hold the same cycles.
void drop_cycle_graphs(ksim_handle* h) {
  drop_graphs_if(h, [](const GraphKey& k) { return k.kind == GraphKind::kCycle; });
  drop_group_graphs(h);
  h->graph_gen++;
}

}  // namespace

namespace ksim_host {

void drop_graphs(ksim_handle* h) {
  drop_graphs_if(h, [](const GraphKey&) { return true; });
  drop_cycle_graphs(h);                            // the group graphs and the generation
}

// The loaded queue, with everything compiled against the rows it was loaded
// on (its buffers are not kept for reuse: ksim_set_profile's narrower form is).
void drop_loaded_pods(ksim_handle* h) {
  h->pod_bufs.clear();
  h->pod_buf_bytes.clear();
  h->d_chosen = nullptr;
  h->dp = DevPods{};
  h->batchable.clear();
  h->topo.clear();
}

bool is_sharded(const ksim_handle* h) { return h->comm != nullptr || h->shard_total != 0; }

int validate_pod(ksim_handle* h, const ksim_pod_set* ps, int32_t i) {
  const ksim_pod& p = ps->pods[i];
  const DevCluster& c = h->dc;
  if (p.flags & (KSIM_POD_HAS_HOST_PORTS | KSIM_POD_HAS_VOLUMES))
    return set_err(h, KSIM_E_UNSUPPORTED, "pod " + std::to_string(i) + ": host ports / volumes not supported by the engine");
  if (p.node_name < -2 || p.node_name >= c.n_total)
    return set_err(h, KSIM_E_INVALID, "pod " + std::to_string(i) + ": node_name out of range");
  auto check_expr = [&](int32_t e) -> bool {
    if (e < 0 || e >= ps->n_exprs) return false;
    const ksim_label_expr& x = ps->exprs[e];
    if (x.nvals > KSIM_EXPR_VALS || x.op > KSIM_OP_TRUE) return false;
    if (x.op <= KSIM_OP_LT && x.col >= c.n_label_cols) return false;
    return true;
  };
  auto check_terms = [&](int32_t first, int32_t count) -> bool {
    if (count < 0 || (count > 0 && (first < 0 || first + count > ps->n_terms))) return false;
    for (int32_t t = 0; t < count; t++) {
      const ksim_term& tm = ps->terms[first + t];
      if (tm.n_expr < 0) return false;
      for (int32_t k = 0; k < tm.n_expr; k++)
        if (!check_expr(tm.first_expr + k)) return false;
    }
    return true;
  };
  if (p.sel_count < 0) return set_err(h, KSIM_E_INVALID, "bad sel_count");
  for (int32_t k = 0; k < p.sel_count; k++)
    if (!check_expr(p.sel_first + k)) return set_err(h, KSIM_E_INVALID, "pod " + std::to_string(i) + ": bad nodeSelector expr");
  if (!check_terms(p.req_term_first, p.req_term_count) || !check_terms(p.pref_term_first, p.pref_term_count))
    return set_err(h, KSIM_E_INVALID, "pod " + std::to_string(i) + ": bad affinity term range");
  if ((p.flags & KSIM_POD_ADDED_AFFINITY) && (p.added_term_count <= 0 || !check_terms(p.added_term_first, p.added_term_count)))
    return set_err(h, KSIM_E_INVALID, "pod " + std::to_string(i) + ": bad addedAffinity term range");
  const std::string who = "pod " + std::to_string(i) + ": ";
  for (const auto& vl : {std::make_pair(p.vb_first, p.vb_count), std::make_pair(p.vz_first, p.vz_count)}) {
    if (vl.second == 0) continue;
    if (!check_terms(vl.first, vl.second)) return set_err(h, KSIM_E_INVALID, who + "bad volume term range");
    for (int32_t k = 0; k < vl.second; k++) {   // group indices: non-negative, non-decreasing
      const int32_t g = ps->terms[vl.first + k].weight;
      if (g < 0 || (k > 0 && g < ps->terms[vl.first + k - 1].weight))
        return set_err(h, KSIM_E_INVALID, who + "volume term groups must be non-decreasing");
    }
  }
  if (p.use_count < 0 || p.use_count > KSIM_MAX_USES ||
      (p.use_count > 0 && (!ps->uses || p.use_first < 0 || p.use_first + p.use_count > ps->n_uses)))
    return set_err(h, KSIM_E_INVALID, who + "bad topology use range");
  for (int32_t k = 0; k < p.use_count; k++) {
    const ksim_topo_use& u = ps->uses[p.use_first + k];
    if (u.kind > KSIM_USE_VOLUME) return set_err(h, KSIM_E_INVALID, who + "bad topology use kind");
    if (u.cls < -1 || u.cls >= c.n_classes) return set_err(h, KSIM_E_INVALID, who + "topology use class out of range");
    if (u.kind == KSIM_USE_VOLUME) {                 // col is a family index, not a label column
      if (is_sharded(h) || h->replicated)
        return set_err(h, KSIM_E_UNSUPPORTED, who + "volume uses run on unsharded handles");
      if (!c.vol_nf) return set_err(h, KSIM_E_INVALID, who + "volume use without a volume table (ksim_set_volume_limits)");
      if (u.col >= c.vol_nf) return set_err(h, KSIM_E_INVALID, who + "volume use family out of range");
      if (u.cls < 0 ? u.arg < 1 : u.arg != 1) return set_err(h, KSIM_E_INVALID, who + "bad volume use count");
      continue;
    }
    if (u.col != KSIM_COL_NONE && u.col >= c.n_label_cols)
      return set_err(h, KSIM_E_INVALID, who + "topology key column out of range");
    if (u.kind == KSIM_USE_PTS_SOFT && c.n_topo_log < c.n + 1)
      return set_err(h, KSIM_E_INVALID, who + "ScheduleAnyway spread needs topo_log[0..n_nodes]");
  }
  if (p.add_count < 0 || (p.add_count > 0 && (!ps->adds || p.add_first < 0 || p.add_first + p.add_count > ps->n_adds)))
    return set_err(h, KSIM_E_INVALID, who + "bad class add range");
  for (int32_t k = 0; k < p.add_count; k++)
    if (ps->adds[p.add_first + k].cls < 0 || ps->adds[p.add_first + k].cls >= c.n_classes)
      return set_err(h, KSIM_E_INVALID, who + "class add out of range");
  if (p.flags & KSIM_POD_NODE_NAMES) {
    if (p.nn_count < 0 || (p.nn_count > 0 && (!ps->nn || p.nn_first < 0 ||
                                              (int64_t)p.nn_first + p.nn_count > (int64_t)ps->n_nn)))
      return set_err(h, KSIM_E_INVALID, who + "bad PreFilterResult node range");
    for (int32_t k = 0; k < p.nn_count; k++) {
      const int32_t v = ps->nn[p.nn_first + k];
      if (v < 0 || v >= c.n_total || (k > 0 && v <= ps->nn[p.nn_first + k - 1]))
        return set_err(h, KSIM_E_INVALID, who + "PreFilterResult nodes must be increasing node positions");
    }
    if (is_sharded(h))
      return set_err(h, KSIM_E_UNSUPPORTED, who + "a PreFilterResult node restriction runs on unsharded handles");
  }
  return KSIM_OK;
}

}  // namespace ksim_host

namespace {

bool plugin_supported(int id) { return id >= 0 && id < KSIM_PL_COUNT; }

// Batch-path eligibility of a pod and the constant it adds to every total.
// The batch path needs P100 (every feasible node is kept, so no window) and
// every normalized plugin constant over nodes:
//   TaintToleration: no PreferNoSchedule taint the pod does not tolerate ->
//                    all raw 0 -> DefaultNormalizeScore(reverse) = 100
//   NodeAffinity:    no preferred terms -> raw 0 -> 0
//   PodTopologySpread: no constraints -> 100
//   InterPodAffinity:  no uses -> topologyScore empty -> 0
//   ImageLocality:     no image use -> 0
// A pod with topology uses reads the count classes, which binds of earlier
// pods of a batch change, so it takes the per-pod path (or the topology
// batches).  An image class is static, so a pod whose only use is its image
// stays here with the score in its keys (pod_batchable).
// Every static filter of the batch path passes on every node for this pod:
// no spec.nodeName, no nodeSelector / required node affinity, every
// NoSchedule/NoExecute taint in the cluster tolerated, no unschedulable node
// (or tolerated).  The batch kernels then skip the static filters.
bool static_trivial(const ksim_handle* h, const ksim_pod& p) {
  if (p.node_name != -1 || p.sel_count > 0 || (p.flags & (KSIM_POD_HAS_REQUIRED_AFFINITY | KSIM_POD_ADDED_AFFINITY)))
    return false;
  if (h->any_unschedulable && !(p.flags & KSIM_POD_TOLERATES_UNSCHEDULABLE)) return false;
  for (uint16_t id : h->hard_taints)
    if (!((p.tol_filter[id >> 6] >> (id & 63)) & 1ull)) return false;
  return true;
}

// The FAST batch kernels (dyn_key_fast): trivial pods, {cpu, memory}
// strategies with weights in [1, 2^31), allocatable cpu / memory below 2^46.
bool run_fast(const ksim_handle* h, int32_t a, int32_t b) {
  if (!h->bp.cpu_mem || !h->bp.fast_w || !h->alloc_narrow) return false;
  for (int32_t i = a; i < b; i++)
    if (!h->trivial[i] || h->batchable[i] == 2) return false;
  return true;
}

// ---- static classes (DevPods::stab) -------------------------------------------
constexpr int32_t kStabMaxClasses = 4096;
constexpr size_t kStabMaxEntries = (size_t)1 << 26;   // 512 MB of table

// The static inputs of a batch pod's keys, as bytes: what static_filters_pass
// (NodeUnschedulable, NodeName, TaintToleration, NodeAffinity) and norm_raw
// read of the pod (its image class among them), the selector and affinity expressions expanded, the
// preferred terms without their weights (two pods with equal signatures have
// equal verdicts, taint counts and preferred-term matches on every node;
// stab_word).  False past 32 preferred terms or for a negative weight.
bool stab_signature(const ksim_pod_set* ps, const ksim_pod& q, std::string& s) {
  s.clear();
  auto put = [&](const void* p, size_t n) { s.append((const char*)p, n); };
  auto put_expr = [&](int32_t e) {
    const ksim_label_expr& x = ps->exprs[e];
    put(&x.num, sizeof x.num);
    put(&x.col, sizeof x.col);
    put(&x.op, sizeof x.op);
    put(&x.nvals, sizeof x.nvals);
    put(x.vals, sizeof(uint32_t) * std::min<int>(x.nvals, KSIM_EXPR_VALS));
  };
  auto put_term = [&](int32_t t, bool preferred) {
    const ksim_term& x = ps->terms[t];
    if (preferred) s.push_back(x.weight != 0 ? 1 : 0);   // a zero weight never counts
    put(&x.n_expr, sizeof x.n_expr);
    for (int32_t k = 0; k < x.n_expr; k++) put_expr(x.first_expr + k);
  };
  const uint32_t fl = q.flags & (KSIM_POD_TOLERATES_UNSCHEDULABLE | KSIM_POD_HAS_REQUIRED_AFFINITY |
                                 KSIM_POD_ADDED_AFFINITY);
  put(&fl, sizeof fl);
  if (q.flags & KSIM_POD_ADDED_AFFINITY) {
    put(&q.added_term_count, sizeof q.added_term_count);
    for (int32_t k = 0; k < q.added_term_count; k++) put_term(q.added_term_first + k, false);
  }
  // the image class of an image pod's one use (-1: none): the word's image
  // field is that class's count column, so image sets never share a class
  const int32_t ic = q.use_count == 1 && ps->uses[q.use_first].kind == KSIM_USE_IMAGE ? ps->uses[q.use_first].cls : -1;
  put(&ic, sizeof ic);
  put(&q.node_name, sizeof q.node_name);
  put(q.tol_filter, sizeof q.tol_filter);
  put(q.tol_prefer, sizeof q.tol_prefer);
  put(&q.sel_count, sizeof q.sel_count);
  for (int32_t k = 0; k < q.sel_count; k++) put_expr(q.sel_first + k);
  put(&q.req_term_count, sizeof q.req_term_count);
  for (int32_t k = 0; k < q.req_term_count; k++) put_term(q.req_term_first + k, false);
  if (q.pref_term_count > 32) return false;
  put(&q.pref_term_count, sizeof q.pref_term_count);
  for (int32_t k = 0; k < q.pref_term_count; k++) {
    put_term(q.pref_term_first + k, true);
    if (ps->terms[q.pref_term_first + k].weight < 0) return false;   // raw scores >= 0 (norm_part_fast)
  }
  return true;
}

// The "ab" flavor: no table (the keys evaluate the static plugins per node).
bool stab_enabled() {
  constexpr bool off = ab(kAbStab);
  return !off;
}

// The static table of the loaded queue's classes on the current snapshot and
// profile, rebuilt in place when stale (in stream order: a graph captured with
// the table replays on the new contents, so a weight sweep keeps its graphs);
// graphs that may hold the table's old address, or a table that no longer
// exists, drop.
int ensure_stab(ksim_handle* h) {
  if (!h->stab_dirty) return KSIM_OK;
  h->stab_dirty = false;
  const bool was_ready = h->stab_ready;
  h->stab_ready = false;
  const size_t entries = (size_t)h->stab_ncls * (size_t)std::max(h->dc.n, 0);
  if (!stab_enabled() || !h->dp.pods || entries == 0 || entries > kStabMaxEntries) {
    if (was_ready) {
      HIPCHK(h, hipStreamSynchronize(h->stream));
      drop_graphs(h);
    }
    return KSIM_OK;
  }
  if (h->stab_bytes < 8 * entries) {
    HIPCHK(h, hipStreamSynchronize(h->stream));
    drop_graphs(h);
    h->stab_bufs.clear();
    h->stab_bytes = 0;
    void* p = nullptr;
    if (const int rc = h->stab_bufs.alloc(h, p, 8 * entries)) return rc;
    h->stab_bytes = 8 * entries;
  } else if (!was_ready) {
    HIPCHK(h, hipStreamSynchronize(h->stream));
    drop_graphs(h);                              // captured without the table
  }
  launch_static_table(make_args(h, h->dp, nullptr), h->d_srep, h->stab_ncls, (uint64_t*)h->stab_bufs[0].p, h->stream);
  HIPCHK(h, hipGetLastError());
  h->stab_ready = true;
  return KSIM_OK;
}

// ADAPT: the profile keeps fewer than all nodes (K < N over the whole cluster).
bool adapt_mode(const ksim_handle* h) {
  return num_feasible_nodes_to_find(h->prof.percentage_of_nodes_to_score, h->dc.n_total) < h->dc.n_total;
}

// The STAB batch kernels (LaunchArgs::stab): every pod of the P100 run in a
// static class, run_fast's cluster conditions, an unsharded handle and the
// default launch forms.
bool run_stab(const ksim_handle* h, int32_t a, int32_t b) {
  if (!h->stab_ready || h->stab_dirty || adapt_mode(h) || is_sharded(h) || h->replicated) return false;
  if (!h->bp.cpu_mem || !h->bp.fast_w || !h->alloc_narrow) return false;
  for (int32_t i = a; i < b; i++)
    if (h->sclass[(size_t)i] < 0) return false;
  return true;
}

// The key kernels of a batch run: FAST, FAST with the static table, or generic.
void pick_keys(const ksim_handle* h, int32_t a, int32_t b, bool& fast, bool& stab) {
  fast = run_fast(h, a, b);
  stab = !fast && run_stab(h, a, b);
  fast = fast || stab;
}

// What a run [a, b) of one handle launches, decided once (plan_run) for
// everything that runs, times or asks about it: run_range, ksim_time_kernels,
// ksim_time_eval, ksim_sweep_loaded.  A form's number is that of the kernel
// family its times are filed under (kFamilies).
enum class RunForm : int {
  kPerPod,       // per-pod cycles (launch_cycle)
  kBatch,        // three-launch P100 batches (launch_batch)
  kAdaptBatch,   // three-launch ADAPT batches (launch_batch_adapt)
  kTbatch,       // topology batches (launch_tbatch)
  kLazy,         // deferred-commit P100 batches (launch_batch_lazy)
  kLazyAdapt,    // deferred-commit ADAPT batches (launch_batch_adapt_lazy)
};

struct RunPlan {
  RunForm form = RunForm::kPerPod;
  bool topo = false;                               // per-pod: the topology kernels run
  bool fast = false, stab = false;                 // LaunchArgs: the batch key kernels (pick_keys)
  bool fuse_min = false, fuse_ext = false, ptab = false;   // LaunchArgs: the per-pod cycle's variants
  bool rt = false;                                 // kLazy: the request-class table (reqtab_ok)
  int family() const { return (int)form; }
  bool lazy() const { return form == RunForm::kLazy || form == RunForm::kLazyAdapt; }
  bool adapt() const { return form == RunForm::kAdaptBatch || form == RunForm::kLazyAdapt; }
};

void apply_plan(const RunPlan& p, LaunchArgs& la) {
  std::tie(la.fast, la.stab, la.fuse_min, la.fuse_ext, la.ptab) = std::tie(p.fast, p.stab, p.fuse_min, p.fuse_ext, p.ptab);
}

// NetworkBandwidth in the profile (Filter or Score)
bool profile_nb(const ksim_profile& p) {
  return prof_has_filter(p, KSIM_PL_NETWORK_BANDWIDTH) || prof_has_score(p, KSIM_PL_NETWORK_BANDWIDTH);
}

// The batch keys carry a pod's total minus its constant normalized part in
// 20 bits (tb_key): 100 * (w_fit + w_ba), plus w_il for a pod with an image
// use and w_tt + w_na for the pods whose normalized scores vary, must stay
// below kKeyTotalLimit, or the pods
// take the per-pod path, whose (total, TB) pairs are exact for any int64 total.  Pods that NodeAffinity's PreFilterResult
// restricts scan a node list of their own: per-pod path.
// A pod's topology uses read count classes that binds of earlier pods of a
// batch change: per-pod path (or the topology batches, tbatch_admit).  The
// exception is a pod whose uses are exactly one KSIM_USE_IMAGE: its
// ImageLocality score is the image class's count column, which no bind
// changes (image classes have no adds) and which needs no NormalizeScore, so
// the keys carry w_il * score as a third static part beside the two
// normalized ones (norm_part; the static-table word holds it, stab_word).
// Returns 0 (per-pod path), 1 (every batch path) or 2 (the unsharded P100
// batch path, and the unsharded ADAPT one without scalar requests:
// pod_on_batch): pods whose TaintToleration / NodeAffinity scores vary
// over nodes (kPodNormVaries: the keys carry them, normalized over the pod's
// S0 maxima), pods with an image use (kPodNormVaries too: the same key sites
// add the image part, and maxima of 0 / 0 never cut such a pod) and pods with
// scalar requests (the ADAPT repair's compact rows carry no scalars).
int pod_batchable(const ksim_handle* h, const ksim_pod& p, const ksim_topo_use* uses, bool* norm_varies = nullptr) {
  const ksim_profile& prof = h->prof;
  if (norm_varies) *norm_varies = false;
  const bool image = p.use_count == 1 && uses && uses[p.use_first].kind == KSIM_USE_IMAGE;
  if (p.use_count > 0 && !image) return 0;
  if (p.flags & KSIM_POD_NODE_NAMES) return 0;
  if (p.vb_count > 0 || p.vz_count > 0) return 0;       // volume groups: the per-pod filter chain
  // NetworkBandwidth runs on the per-pod path (its error statuses end cycles),
  // and so do pods that add to a node's allocated bandwidth
  if (profile_nb(prof) || p.nb_add != 0) return 0;
  const int64_t w_dyn = h->bp.w_fit + h->bp.w_ba;
  if ((int64_t)kMaxNodeScore * w_dyn >= kKeyTotalLimit) return 0;
  int cls = (p.flags & KSIM_POD_HAS_SCALAR) ? 2 : 1;
  bool varies = false;
  for (int k = 0; k < prof.n_score; k++) {
    switch (norm_kind(prof.score[k])) {
      case kNormDefaultReverse:                         // varies when some PreferNoSchedule taint is not tolerated
        for (size_t t = 1; t < h->taint_effect.size(); t++)
          if (h->taint_effect[t] == KSIM_EFFECT_PREFER_NO_SCHEDULE && !((p.tol_prefer[t >> 6] >> (t & 63)) & 1ull))
            varies = true;
        break;                                          // else every node 100
      case kNormDefault:
        if (p.pref_term_count > 0) varies = true;        // else every node 0
        break;
      default:                                          // PodTopologySpread 100, InterPodAffinity 0
        break;
    }
  }
  const int64_t w_img = image ? h->bp.w_il : 0;
  if ((int64_t)kMaxNodeScore * (w_dyn + w_img + (varies ? h->bp.w_tt + h->bp.w_na : 0)) >= kKeyTotalLimit) return 0;
  varies = varies || image;
  if (varies) cls = 2;
  if (norm_varies) *norm_varies = varies;
  return cls;
}

// Whether loaded pod i runs on this handle's batch path (see pod_batchable):
// class 2 needs the unsharded P100 path over the whole node table.
// Class 2 under ADAPT: pods whose normalized scores vary (k_adapt_top's
// maxima over the window's kept nodes), without scalar requests, on an
// unsharded handle (the "ab" flavor: the per-pod path).
bool pod_on_batch(const ksim_handle* h, int32_t i) {
  constexpr bool adapt_norm = !ab(kAbAdaptNorm);
  const uint8_t b = h->batchable[i];
  if (b != 2 && b != 3) return b != 0;
  if (h->replicated) return b == 3 && !adapt_mode(h);   // class 3: replicated topology batches (shard_run_tbatch)
  if (is_sharded(h)) return false;
  if (!adapt_mode(h)) return true;
  return b == 2 && adapt_norm && h->noscalar[(size_t)i];
}

// Topology pods the topology batch path takes (class 3; ksim_tbatch.hip): the
// per-pod path's fused no-window cycle would run them (at most one
// ScheduleAnyway spread constraint, keyed by hostname or by no node's key;
// hard spread keys of <= kFuseMinValues values) with every domain sum read
// from a persistent table, no port / volume / bandwidth inputs and no
// PreFilterResult node list, totals inside the batch key's 20 bits, and a
// cluster of at most kTbMaxBlocks node blocks.  The "ab" flavor: per-pod path.
bool tbatch_admit(const ksim_handle* h, const ksim_pod& p, const PodPlan& pl, bool hard_small, bool soft_le1) {
  constexpr bool off = ab(kAbTbatch);
  if (off || p.use_count <= 0) return false;
  if (h->dc.n > kTbMaxBlocks * 256) return false;
  if (p.flags & KSIM_POD_NODE_NAMES) return false;
  if (p.vb_count > 0 || p.vz_count > 0 || profile_nb(h->prof) || p.nb_add != 0) return false;
  const UseMasks& m = pl.m;
  if (m.port || m.vol || m.soft_val || !hard_small || !soft_le1) return false;
  const bool pt = (pl.flags & kPlanPtab) != 0;
  if ((m.dom & ~(pt ? m.ptab : 0u)) != 0) return false;     // a domain sum k_topo_prefilter would build
  if ((m.aff | m.score) != 0 && !pt) return false;         // the InterPodAffinity flags come from the tables
  int64_t wsum = 0;
  for (int k = 0; k < h->prof.n_score; k++) wsum += h->prof.score_weight[k] == 0 ? 1 : h->prof.score_weight[k];
  return (int64_t)kMaxNodeScore * wsum < kKeyTotalLimit;
}

// A framework-driven cycle left behind by another entry point: its PreFilter
// domain sums were never re-zeroed by a k_select (no ksim_fw_score ran), and
// its pod / scratch state is about to be replaced.
int fw_abandon(ksim_handle* h) {
  if (h->fw_dom_dirty && h->sc.dom)
    HIPCHK(h, hipMemsetAsync(h->sc.dom, 0, 8 * (size_t)KSIM_MAX_USES * h->dc.vmax, h->stream));
  h->fw_dom_dirty = h->fw_pending = h->fw_scored = false;
  h->fw_list.clear();
  h->fw_raw.clear();
  return KSIM_OK;
}

}  // namespace
static int flush_deferred_binds(ksim_handle* h);
// The queued Reserve of the last framework cycle (pend_bind), launched now.
int ksim_host::flush_pend_bind(ksim_handle* h) {
  if (!h || !h->pend_bind.on) return KSIM_OK;
  h->pend_bind.on = false;
  HIPCHK(h, hipSetDevice(h->device));
  launch_assume(h->dc, h->pend_bind.P, 0, h->pend_bind.node, h->pend_bind.sign, h->stream);
  HIPCHK(h, hipGetLastError());
  return KSIM_OK;
}
namespace ksim_host {

int ensure_ready(ksim_handle* h, bool fw, bool keep_pend) {
  if (!h) return KSIM_E_INVALID;
  if (!keep_pend) {
    const int rc = flush_pend_bind(h);
    if (rc) return rc;
  }
  if (!fw && (h->fw_pending || h->fw_scored || h->fw_dom_dirty)) {
    const int rc = fw_abandon(h);
    if (rc) return rc;
  }
  if (!h->has_profile) return set_err(h, KSIM_E_INVALID, "profile not set");
  if (!h->has_cluster) return set_err(h, KSIM_E_INVALID, "cluster not set");
  if (h->dc.n <= 0) return set_err(h, KSIM_E_INVALID, "no nodes available");
  if (!h->fw_pending && !h->deferred_binds.empty()) return flush_deferred_binds(h);
  return KSIM_OK;
}

LaunchArgs make_args(ksim_handle* h, const DevPods& P, int32_t* chosen) {
  LaunchArgs a;
  a.c = h->dc;
  a.c.eval_lo = 0;                       // every node (replicated shard batches narrow it, shard_batch)
  a.c.eval_hi = a.c.n;
  a.c.count_whole = (!h->replicated || h->rep_primary) ? 1 : 0;
  a.P = P;
  if (h->stab_ready && !h->stab_dirty && P.pods == h->dp.pods) {   // the loaded queue's static classes
    a.P.sclass = h->d_sclass;
    a.P.stab = (const uint64_t*)h->stab_bufs[0].p;
    a.P.stab_fast = (h->bp.cpu_mem && h->bp.fast_w && h->alloc_narrow) ? 1 : 0;
  }
  a.prof = h->prof;
  a.bp = h->bp;
  a.dprof = h->d_prof;
  a.dbp = h->d_bp;
  a.st = h->st;
  a.s = h->sc;
  a.o = h->eo;
  a.chosen = chosen;
  return a;
}

int set_run(ksim_handle* h, int32_t first, int32_t end) {
  h->run_hdr[0] = first;
  h->run_hdr[1] = end;
  HIPCHK(h, hipMemcpyAsync(h->st, h->run_hdr, sizeof(h->run_hdr), hipMemcpyHostToDevice, h->stream));
  // a run starts with full batches (generic ADAPT batches cap the next one, DevState::bcap)
  HIPCHK(h, hipMemsetAsync(&h->st->bcap, 0, sizeof(int32_t), h->stream));
  // per-cycle selection state starts from zero (the no-window cycle keeps it
  // zero between its own cycles; other paths leave extrema behind)
  HIPCHK(h, hipMemsetAsync(h->sc.win, 0, sizeof(WinState), h->stream));
  return KSIM_OK;
}

}  // namespace ksim_host

namespace {

int read_state_at(ksim_handle* h, const DevState* src, DevState& st) {
  HIPCHK(h, hipMemcpyAsync(&st, src, sizeof(st), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return KSIM_OK;
}

int read_state(ksim_handle* h, DevState& st) { return read_state_at(h, h->st, st); }

// reps x body(i) on `stream` (idle: the caller has synchronised it) as an
// instantiated graph in *out.  body returns KSIM_OK or a code; a capture that
// began is always ended.  On failure *out is null and `what` names the call
// that failed (a body that failed reads as an invalidated capture).
template <class B>
hipError_t capture_graph(hipStream_t stream, int reps, B&& body, hipGraphExec_t* out, const char*& what) {
  *out = nullptr;
  what = "hipStreamBeginCapture";
  hipError_t e = hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal);
  if (e != hipSuccess) return e;
  bool ok = true;
  for (int i = 0; ok && i < reps; i++) ok = body(i) == KSIM_OK;
  hipGraph_t g = nullptr;
  what = "hipStreamEndCapture";
  e = hipStreamEndCapture(stream, &g);            // ends a capture even after a failed launch
  if (e == hipSuccess && !(ok && g)) e = hipErrorStreamCaptureInvalidated;
  if (e == hipSuccess) {
    what = "hipGraphInstantiate";
    e = hipGraphInstantiate(out, g, nullptr, nullptr, 0);
    if (e != hipSuccess) *out = nullptr;
  }
  if (g) (void)hipGraphDestroy(g);
  return e;
}

// A single handle's graph of reps x launch(i): a failure is the handle's error.
template <class L>
int capture_launches(ksim_handle* h, int reps, L&& launch, hipGraphExec_t* out) {
  const char* what;
  const hipError_t e = capture_graph(h->stream, reps, [&](int i) { return launch(i), (int)KSIM_OK; }, out, what);
  if (e != hipSuccess) return hip_fail(h, e, what);
  h->graph_captures++;
  return KSIM_OK;
}

// The handle's graph under `key`: the cached one, or (unless !may_capture:
// then none) reps x launch(i) captured now on the synchronised stream and kept.
// A failed capture leaves no entry.  Runs look their graph up once, at their start.
template <class L>
int handle_graph(ksim_handle* h, const GraphKey& key, int reps, L&& launch, hipGraphExec_t* out,
                 bool may_capture = true) {
  const auto it = h->graphs.find(key);
  *out = it == h->graphs.end() ? nullptr : it->second;
  if (*out || !may_capture) return KSIM_OK;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (int rc = capture_launches(h, reps, launch, out)) return rc;
  h->graphs.emplace(key, *out);
  return KSIM_OK;
}

// The state a run of topology batches starts from (run_tbatch, ksim_time_kernels).
int tbatch_begin(ksim_handle* h) {
  HIPCHK(h, hipMemsetAsync(h->sc.tb_win, 0, sizeof(WinState) * kTbPods, h->stream));
  HIPCHK(h, hipMemsetAsync(h->sc.tb_dom, 0, sizeof(TbDom) * kTbPods * kVarDom, h->stream));
  HIPCHK(h, hipMemsetAsync(h->sc.tb_vhold, 0, 4 * (size_t)kTbPods * kVarSlots * 2 * KSIM_MAX_SCORE, h->stream));
  return KSIM_OK;
}

// A run of topology batch pods [a, b) (set_run done).  The host knows each
// batch's pod count (the conflict-free run from its first pod, capped) and a
// batch commits at most that many, so launching the batches the counts predict
// never passes the end; a batch that commits fewer (a cut, an exhausted list,
// pinv) leaves pods for the next round.
int run_tbatch(ksim_handle* h, int32_t a, int32_t b, const LaunchArgs& la) {
  int rc;
  if ((rc = tbatch_begin(h))) return rc;
  hipGraphExec_t graph;
  if ((rc = handle_graph(h, {GraphKind::kTbatch, {}}, kGraphBatches, [&](int) { launch_tbatch(la, h->stream); }, &graph)))
    return rc;
  int32_t cursor = a;
  while (cursor < b) {
    int32_t nbat = 0;
    for (int32_t i = cursor; i < b; nbat++) i += std::min(std::min(kTbPods, b - i), std::max(h->tlen[i], 1));
    int32_t done = 0;
    for (; done + kGraphBatches <= nbat; done += kGraphBatches) HIPCHK(h, hipGraphLaunch(graph, h->stream));
    for (; done < nbat; done++) launch_tbatch(la, h->stream);
    HIPCHK(h, hipGetLastError());
    DevState st;
    if ((rc = read_state(h, st))) return rc;
    if (st.cursor <= cursor) return set_err(h, KSIM_E_DEVICE, "topology batch path made no progress");
    cursor = st.cursor;
  }
  return KSIM_OK;
}

// ---- deferred-commit FAST batches (ksim_internal.h, ksim_batch.hip) ----------
// The "ab" flavor: the three-launch batches (parity of both forms).
bool lazy_enabled() {
  constexpr bool off = ab(kAbLazy);
  return !off;
}

// A FAST run [a, b) whose pods add to no count class (the overlay carries the
// resource columns only), on a cluster the overlay's LDS node bitmap covers.
// Generic runs and static-class runs keep the three launches: the deferred
// commit measured slower for both (config 1 scaled, profiles/r03/ab_lazy_gen:
// 46.8 against 35.3 ms per step for generic keys, whose loop with the overlay
// held 205 VGPRs; profiles/r03/ab_stab: 13.3 against 12.7 ms for the
// static-class keys, whose overlay lookups in both passes cost more than the
// commit launch).
bool lazy_ok(const ksim_handle* h, int32_t a, int32_t b, bool fast, bool stab = false) {
  if (!lazy_enabled() || !fast || stab) return false;
  // ADAPT runs whole on a replica (no exchange); replicated P100 batches take
  // shard_run_lazy (lazy_rep_ok)
  if (adapt_mode(h) ? (is_sharded(h) && !h->replicated) : (is_sharded(h) || h->replicated)) return false;
  if (h->dc.base != 0 || h->dc.n > kLazyMaxNodes || h->dc.n <= 0) return false;
  for (int32_t i = a; i < b; i++)
    if (!h->noadd[i]) return false;
  return true;
}

// KSIM_ONE_CUT=1 (read at every run, as KSIM_FEED_FLUSH): every deferred-commit
// batch ends at its first pair cut, the rule before the second stretch
// (ksim_batch.hip; an A/B form of the same runs).  The setting is a launch
// argument (LazyStep::one_cut), so the graphs captured under the other one go.
int sync_one_cut(ksim_handle* h) {
  const char* v = std::getenv("KSIM_ONE_CUT");
  const bool want = v && v[0] == '1';
  if (want == h->one_cut) return KSIM_OK;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  drop_graphs_if(h, [](const GraphKey& k) { return k.kind == GraphKind::kLazy || k.kind == GraphKind::kSweep; });
  drop_group_graphs(h);                           // a replica group's (its leader's)
  h->one_cut = want;
  return KSIM_OK;
}

int alloc_lazy(ksim_handle* h) {
  if (int rc = sync_one_cut(h)) return rc;
  if (h->lazy.n == h->dc.n) return KSIM_OK;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  drop_graphs_if(h, is_lazy);
  h->lazy = LazyBufs{};
  if (!h->prog.p) {   // reserved once, at one size: the graphs hold its address (the stream is idle, above)
    if (const int rc = h->prog.reserve(h, 2 * sizeof(unsigned long long), Idle::kCaller)) return rc;
    std::memset(h->prog.p, 0, 2 * sizeof(unsigned long long));
  }
  const size_t n = (size_t)h->dc.n;
  int rc;
  int64_t** cols[5] = {&h->lazy.x1.req_cpu, &h->lazy.x1.req_mem, &h->lazy.x1.req_eph, &h->lazy.x1.nz_cpu,
                       &h->lazy.x1.nz_mem};
  for (auto* c : cols)
    if ((rc = h->lazy.bufs.alloc(h, *c, 8 * n))) return rc;
  if ((rc = h->lazy.bufs.alloc(h, h->lazy.x1.num_pods, 4 * n)) ||
      (rc = h->lazy.bufs.alloc(h, h->lazy.st1, sizeof(DevState))) ||
      (rc = h->lazy.bufs.alloc(h, h->lazy.g, 8 * (size_t)kLazySlots * kBatchPods)) ||
      (rc = h->lazy.bufs.alloc(h, h->lazy.m, 8 * (size_t)kLazySlots * kBatchPods)) ||
      (rc = h->lazy.bufs.alloc(h, h->lazy.e, 4 * (size_t)kLazySlots)) ||
      (rc = h->lazy.bufs.alloc(h, h->lazy.ab, 4 * (size_t)kLazySlots * kBatchPods)) ||
      (rc = h->lazy.bufs.alloc(h, h->lazy.aw, 8 * (size_t)kLazySlots * kBatchPods)))
    return rc;
  h->lazy.n = h->dc.n;
  return KSIM_OK;
}

DynCols dyn_cols(const DevCluster& c) {
  return DynCols{c.req_cpu, c.req_mem, c.req_eph, c.nz_cpu, c.nz_mem, c.num_pods};
}

DevCluster with_cols(DevCluster c, const DynCols& d) {
  c.req_cpu = d.req_cpu;
  c.req_mem = d.req_mem;
  c.req_eph = d.req_eph;
  c.nz_cpu = d.nz_cpu;
  c.nz_mem = d.nz_mem;
  c.num_pods = d.num_pods;
  return c;
}

// ---- request classes (ksim_internal.h ReqTab) ----------------------------------
// The "ab" flavor: every pod x node pair keyed (today's KEEP / DEF kernel).
bool reqtab_enabled() {
  constexpr bool off = ab(kAbReqTab);
  return !off;
}

// A deferred-commit P100 run [a, b) (lazy_ok holds) takes the table where
// k_batch_top_commit<false, true, true, true> runs (fast_def, the KEEP range),
// with every pod in a request class, at most kReqMaxClasses of them, and at
// least 8 pods per class: the build keys C x N pairs and every batch's upkeep
// up to 2 B C more, so a run not much longer than C gains nothing.
bool reqtab_ok(const ksim_handle* h, int32_t a, int32_t b) {
  if (!reqtab_enabled() || adapt_mode(h) || !fast_def(h->bp)) return false;
  if (h->dc.n > kKeepPerLane * 1024) return false;   // the KEEP range (within the direct overlay's)
  const int32_t C = h->rq_ncls;
  if (C <= 0 || C > kReqMaxClasses || (int64_t)(b - a) < 8 * (int64_t)C || !h->d_rcls) return false;
  for (int32_t i = a; i < b; i++)
    if (h->rq_cls[(size_t)i] == 0xffff) return false;
  return true;
}

// The plan of run [a, b), one of for_each_run's (batch, topo: its path).
RunPlan plan_run(const ksim_handle* h, int32_t a, int32_t b, bool batch, bool topo) {
  RunPlan p;
  if (!batch) {
    p.topo = topo;
    p.fuse_min = topo;
    for (int32_t i = a; i < b && p.fuse_min; i++) p.fuse_min = h->hard_small[i] != 0;
    p.fuse_ext = true;
    for (int32_t i = a; i < b && p.fuse_ext; i++) p.fuse_ext = h->soft_le1[i] != 0;
    p.ptab = h->topo[a] == 2;                      // runs are uniform in topo (for_each_run)
  } else if (topo) {
    p.form = RunForm::kTbatch;
  } else {
    // the FAST evaluation kernel when every pod of the run is trivial with
    // cpu/memory scoring, or is in a static class (STAB)
    pick_keys(h, a, b, p.fast, p.stab);
    const bool adapt = adapt_mode(h);
    if (lazy_ok(h, a, b, p.fast, p.stab)) {
      p.form = adapt ? RunForm::kLazyAdapt : RunForm::kLazy;
      p.rt = reqtab_ok(h, a, b);
    } else {
      p.form = adapt ? RunForm::kAdaptBatch : RunForm::kBatch;
    }
  }
  return p;
}

// The table's two halves for the handle's cluster, then (at a 256-byte step)
// the ring's patch entries P[kLazySlots][C][kBatchPods]; a reallocation drops
// the graph that holds their addresses (ensure_stab's rule).  Behind them (a
// slot is a multiple of 512 bytes) the pod records H[2][2 * kBatchPods].
size_t rtab_halves_bytes(const ksim_handle* h) {
  const size_t t = 2 * sizeof(uint16_t) * (size_t)h->rq_ncls * (size_t)h->dc.n;
  return (t + 255) & ~(size_t)255;
}
size_t rtab_patch_bytes(const ksim_handle* h) {
  return sizeof(uint16_t) * kLazySlots * (size_t)h->rq_ncls * kBatchPods;
}
int ensure_rtab(ksim_handle* h) {
  const size_t need = rtab_halves_bytes(h) + rtab_patch_bytes(h) + sizeof(PodRec) * 2 * 2 * kBatchPods;
  if (h->rtab_bytes >= need && !h->rtab_bufs.empty()) return KSIM_OK;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  drop_graphs_if(h, is_table);
  h->rtab_bufs.clear();
  h->rtab_bytes = 0;
  void* p = nullptr;
  if (const int rc = h->rtab_bufs.alloc(h, p, need)) return rc;
  h->rtab_bytes = need;
  return KSIM_OK;
}

// The launch arguments of deferred-commit batch i of a run (rt: with the
// request-class table, ensure_rtab done).
LazyBatch lazy_batch(const ksim_handle* h, const LaunchArgs& la, int64_t i, bool rt = false) {
  const int p = (int)(i & 1), q = (int)(i & 3), q1 = (int)((i + 3) & 3), q2 = (int)((i + 2) & 3);
  const DynCols x[2] = {dyn_cols(h->dc), h->lazy.x1};
  DevState* st[2] = {h->st, h->lazy.st1};
  LazyBatch z;
  z.a = la;
  z.a.c = with_cols(la.c, x[p ^ 1]);
  z.cw = with_cols(la.c, x[p]);
  z.step.w = x[p];
  z.step.st_in = st[p ^ 1];
  z.step.st_out = st[p];
  z.step.g1 = h->lazy.g + (size_t)q1 * kBatchPods;
  z.step.m1 = h->lazy.m + (size_t)q1 * kBatchPods;
  z.step.e1 = h->lazy.e + q1;
  z.step.g2 = h->lazy.g + (size_t)q2 * kBatchPods;
  z.step.e2 = h->lazy.e + q2;
  z.step.e_self = h->lazy.e + q;
  z.step.prog = (unsigned long long*)h->prog.d;
  z.step.one_cut = h->one_cut ? 1 : 0;
  z.st = st[p];
  z.gkey = h->lazy.g + (size_t)q * kBatchPods;
  z.pmax = h->lazy.m + (size_t)q * kBatchPods;
  z.cend = h->lazy.e + q;
  z.b1 = h->lazy.ab + (size_t)q1 * kBatchPods;
  z.w1 = h->lazy.aw + (size_t)q1 * 2 * kBatchPods;
  z.abroken = h->lazy.ab + (size_t)q * kBatchPods;
  z.awin = h->lazy.aw + (size_t)q * 2 * kBatchPods;
  if (rt) {
    uint16_t* const t = (uint16_t*)h->rtab_bufs[0].p;
    const size_t half = (size_t)h->rq_ncls * (size_t)h->dc.n;
    z.rt.t_in = t + (size_t)(p ^ 1) * half;
    z.rt.t_out = t + (size_t)p * half;
    z.rt.rreq = h->d_rreq;
    z.rt.rcls = h->d_rcls;
    z.rt.n_cls = h->rq_ncls;
    // the patch entries: batch i's pairs launch writes slot q, batch i's
    // evaluation launch reads batch i-1's
    uint16_t* const pe = (uint16_t*)((char*)h->rtab_bufs[0].p + rtab_halves_bytes(h));
    const size_t slot = (size_t)h->rq_ncls * kBatchPods;
    z.rt.p_in = pe + (size_t)q1 * slot;
    z.rt.p_out = pe + (size_t)q * slot;
    // the pod records: batch i's evaluation launch reads batch i-1's and writes its own
    PodRec* const rec = (PodRec*)((char*)pe + rtab_patch_bytes(h));
    z.rt.h_in = rec + (size_t)(p ^ 1) * 2 * kBatchPods;
    z.rt.h_out = rec + (size_t)p * 2 * kBatchPods;
  }
  return z;
}

// Start of a deferred-commit run (set_run done): X[1] = X[0], st[1] = st[0],
// every ring slot empty.
int lazy_begin(ksim_handle* h) {
  int rc;
  if ((rc = alloc_lazy(h))) return rc;
  const size_t n = (size_t)h->dc.n;
  const DynCols x0 = dyn_cols(h->dc), x1 = h->lazy.x1;
  HIPCHK(h, hipMemcpyAsync(x1.req_cpu, x0.req_cpu, 8 * n, hipMemcpyDeviceToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(x1.req_mem, x0.req_mem, 8 * n, hipMemcpyDeviceToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(x1.req_eph, x0.req_eph, 8 * n, hipMemcpyDeviceToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(x1.nz_cpu, x0.nz_cpu, 8 * n, hipMemcpyDeviceToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(x1.nz_mem, x0.nz_mem, 8 * n, hipMemcpyDeviceToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(x1.num_pods, x0.num_pods, 4 * n, hipMemcpyDeviceToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(h->lazy.st1, h->st, sizeof(DevState), hipMemcpyDeviceToDevice, h->stream));
  HIPCHK(h, hipMemsetAsync(h->lazy.e, 0xff, 4 * kLazySlots, h->stream));
  return KSIM_OK;
}

// After the flush of batch index f: the snapshot and state are in X[f & 1],
// st[f & 1]; bring them to the handle's own buffers.
int lazy_end(ksim_handle* h, int64_t f) {
  if ((f & 1) == 0) return KSIM_OK;
  const size_t n = (size_t)h->dc.n;
  const DynCols x0 = dyn_cols(h->dc), x1 = h->lazy.x1;
  HIPCHK(h, hipMemcpyAsync(x0.req_cpu, x1.req_cpu, 8 * n, hipMemcpyDeviceToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(x0.req_mem, x1.req_mem, 8 * n, hipMemcpyDeviceToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(x0.req_eph, x1.req_eph, 8 * n, hipMemcpyDeviceToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(x0.nz_cpu, x1.nz_cpu, 8 * n, hipMemcpyDeviceToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(x0.nz_mem, x1.nz_mem, 8 * n, hipMemcpyDeviceToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(x0.num_pods, x1.num_pods, 4 * n, hipMemcpyDeviceToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(h->st, h->lazy.st1, sizeof(DevState), hipMemcpyDeviceToDevice, h->stream));
  return KSIM_OK;
}

// A run of pods [a, b) as deferred-commit batches (lazy_ok; set_run done).
// Batch i commits batch i - 1; each stretch of launches ends with a flush, whose
// state tells the host where the run stands.  A batch commits 1..kBatchPods
// pods, so ceil(left / kBatchPods) batches never start past the end.
uint32_t lazy_launch(const ksim_handle* h, const LazyBatch& z, hipStream_t stream, hipEvent_t* evs = nullptr) {
  return adapt_mode(h) ? launch_batch_adapt_lazy(z, stream, evs) : launch_batch_lazy(z, stream, evs);
}

void lazy_flush(const ksim_handle* h, const LazyBatch& z, hipStream_t stream) {
  if (adapt_mode(h)) launch_adapt_lazy_flush(z, stream);
  else launch_lazy_flush(z, stream);
}

// Both halves of the table from the run's starting snapshot (lazy_begin done),
// and the pod records batch 0's evaluation launch reads: those of the run's
// first pods (nothing in H is kept from an earlier run).
int reqtab_begin(ksim_handle* h, const LaunchArgs& la, int32_t first, int32_t end) {
  int rc;
  if ((rc = ensure_rtab(h))) return rc;
  const LazyBatch z0 = lazy_batch(h, la, 0, true);
  launch_req_table(la, z0.rt, z0.rt.t_out, const_cast<uint16_t*>(z0.rt.t_in), h->stream);
  launch_req_records(la, z0.rt, first, end, const_cast<PodRec*>(z0.rt.h_in), h->stream);
  return KSIM_OK;
}

// run_lazy's begin in one launch (k_lazy_move): reset_counters when the call's
// counters are still to zero, set_run and lazy_begin.
int lazy_begin_run(ksim_handle* h, int32_t first, int32_t end, bool zero_counters) {
  int rc;
  if ((rc = alloc_lazy(h))) return rc;
  h->run_hdr[0] = first;
  h->run_hdr[1] = end;
  LazyMove m{};
  m.src = dyn_cols(h->dc);
  m.dst = h->lazy.x1;
  m.n = h->dc.n;
  m.begin = 1;
  m.zero_counters = zero_counters ? 1 : 0;
  m.first = first;
  m.end = end;
  m.st_src = h->st;
  m.st_dst = h->st;
  m.st_dst2 = h->lazy.st1;
  m.win = h->sc.win;
  m.ring_e = h->lazy.e;
  m.batches0 = (unsigned long long*)h->prog.d + 1;
  launch_lazy_move(m, h->stream);
  HIPCHK(h, hipGetLastError());
  return KSIM_OK;
}

// lazy_end in one launch.
int lazy_end_run(ksim_handle* h, int64_t f) {
  if ((f & 1) == 0) return KSIM_OK;
  LazyMove m{};
  m.src = h->lazy.x1;
  m.dst = dyn_cols(h->dc);
  m.n = h->dc.n;
  m.st_src = h->lazy.st1;
  m.st_dst = h->st;
  launch_lazy_move(m, h->stream);
  HIPCHK(h, hipGetLastError());
  return KSIM_OK;
}

// KSIM_FEED_FLUSH=1 (read at every run): every stretch ends with a flush and
// a synchronised state read, the loop's fallback taken unconditionally (an
// A/B form of the same runs, and the fallback's test).
bool feed_flush_forced() {
  const char* v = std::getenv("KSIM_FEED_FLUSH");
  return v && v[0] == '1';
}

// The host enqueues batches while none can start past the end, from the
// freshest commit it knows: the state writer of every evaluation launch and of
// every flush stores (cursor, batches) to the handle's progress word, which the
// host polls while the device works, so the stream is topped up without a
// flush, a state read and a synchronisation per stretch.  Only the last
// enqueued batch, when it may end the run, is committed by a flush, whose word
// the host waits for.  A word that does not move within the deadline (sized by
// the launches outstanding) ends the stretch the old way: a flush, a state
// read, a synchronisation.  zero_counters: the begin launch zeroes the call's
// counters (run_range).  plan: the run's (a deferred-commit form).
int run_lazy(ksim_handle* h, int32_t a, int32_t b, const RunPlan& plan, const LaunchArgs& la, bool zero_counters) {
  int rc;
  if ((rc = alloc_lazy(h))) return rc;
  volatile unsigned long long* const word = (unsigned long long*)h->prog.p;
  constexpr unsigned long long kNoWord = ~0ull;     // no cursor is -1
  word[0] = kNoWord;                                // nothing in flight writes it: every run ends waited for
  if ((rc = lazy_begin_run(h, a, b, zero_counters))) return rc;
  // the request-class table, rebuilt from the run's starting snapshot in
  // stream order: anything may have moved X since the last run
  const bool rt = plan.rt;
  if (rt) {
    h->rtab_runs++;
    if ((rc = reqtab_begin(h, la, a, b))) return rc;
  }
  // the run's graph and its tail graph, both from ring phase 0, captured together
  const int32_t adapt = plan.adapt(), ncls = rt ? h->rq_ncls : 0;
  hipGraphExec_t graph, graph4;
  const auto batch_i = [&](int i) { lazy_launch(h, lazy_batch(h, la, i, rt), h->stream); };
  if ((rc = handle_graph(h, {GraphKind::kLazy, {adapt, ncls, 0}}, kGraphBatches, batch_i, &graph)) ||
      (rc = handle_graph(h, {GraphKind::kLazy, {adapt, ncls, 1}}, kLazySlots, batch_i, &graph4)))
    return rc;
  static_assert(kGraphBatches % kLazySlots == 0, "lazy graphs keep the ring phase");
  const bool forced = feed_flush_forced();
  int64_t i = 0;                  // the next launch's ring index (flushes take one)
  int32_t launched = 0, done = 0; // the run's batches enqueued; committed as far as the host has seen
  int32_t cursor = a;             // ... and the cursor after those commits
  bool flushed = false;           // a flush is the last launch enqueued
  unsigned long long last = kNoWord;
  // nb more batches: single launches to the ring phase 0, whole graphs, tail
  // graphs, single launches for the rest
  auto enqueue = [&](int32_t nb) -> int {
    const int32_t align = (int32_t)((kLazySlots - (i & 3)) & 3);
    if (nb >= align + kLazySlots) {
      for (int32_t r = 0; r < align; r++, i++, nb--) lazy_launch(h, lazy_batch(h, la, i, rt), h->stream);
      launched += align;
      for (; nb >= kGraphBatches; nb -= kGraphBatches, i += kGraphBatches, launched += kGraphBatches)
        HIPCHK(h, hipGraphLaunch(graph, h->stream));
      for (; nb >= kLazySlots; nb -= kLazySlots, i += kLazySlots, launched += kLazySlots)
        HIPCHK(h, hipGraphLaunch(graph4, h->stream));
    }
    for (; nb > 0; nb--, i++, launched++) lazy_launch(h, lazy_batch(h, la, i, rt), h->stream);
    HIPCHK(h, hipGetLastError());
    flushed = false;
    return KSIM_OK;
  };
  // What the commits seen so far allow: more batches, and the flush behind the
  // one batch outstanding when no batch may follow it before its commit is
  // known (it may end the run; the first evaluation launch behind a flush
  // repeats the flush's word, so the host does not wait for it).
  auto act = [&](bool top_up) -> int {
    const int32_t pending = launched - done;
    const int32_t more = lazy_more_batches(b - cursor, pending, kBatchPods);
    const int32_t align = (int32_t)((kLazySlots - (i & 3)) & 3);
    // (a whole graph's worth at once; a tail graph's only with less than a
    // graph still queued; single launches only when the stream is about to run dry)
    if (more > 0 && (more >= align + kGraphBatches || (more >= align + kLazySlots && pending <= kGraphBatches - kLazySlots) ||
                     pending <= 2)) {
      if (int r = enqueue(more)) return r;
      if (top_up) h->feed_topups++;
    }
    if (!forced && !flushed && launched - done == 1 && lazy_more_batches(b - cursor, 1, kBatchPods) == 0) {
      lazy_flush(h, lazy_batch(h, la, i, rt), h->stream);
      HIPCHK(h, hipGetLastError());
      i++;
      flushed = true;
    }
    return KSIM_OK;
  };
  if ((rc = act(false))) return rc;
  while (cursor < b) {
    // the word's next value, or none by the deadline
    bool news = false;
    if (!forced) {
      const auto deadline = std::chrono::steady_clock::now() +
                            std::chrono::milliseconds(50 + 5 * (int64_t)(launched - done + 1));
      for (uint32_t spin = 1;; spin++) {
        const unsigned long long w = word[0];
        if (w != last) {
          last = w;
          news = true;
          break;
        }
        if ((spin & 1023) == 0) {
          // a wait far longer than a batch: an error ends the loop, with no
          // launch behind it (no query on the usual path: it may enqueue a
          // marker behind the batches)
          if ((spin & 16383) == 0) {
            const hipError_t q = hipStreamQuery(h->stream);
            if (q != hipSuccess && q != hipErrorNotReady) return hip_fail(h, q, "hipStreamQuery");
          }
          if (std::chrono::steady_clock::now() > deadline) break;
        }
        __builtin_ia32_pause();
      }
    }
    if (news) {
      cursor = (int32_t)(last >> 32);
      done = (int32_t)((uint32_t)last - (uint32_t)word[1]);
    } else {
      // the stretch ends with a flush and a state read (none behind an error)
      if (!forced) {
        const hipError_t q = hipStreamQuery(h->stream);
        if (q != hipSuccess && q != hipErrorNotReady) return hip_fail(h, q, "hipStreamQuery");
      }
      lazy_flush(h, lazy_batch(h, la, i, rt), h->stream);
      HIPCHK(h, hipGetLastError());
      DevState st;
      if ((rc = read_state_at(h, (i & 1) ? h->lazy.st1 : h->st, st))) return rc;
      h->feed_syncs++;
      h->feed_fallbacks++;
      i++;
      flushed = true;
      last = word[0];
      if (st.cursor <= cursor) return set_err(h, KSIM_E_DEVICE, "deferred-commit batch path made no progress");
      cursor = st.cursor;
      done = launched;
    }
    if (cursor < b && (rc = act(true))) return rc;
  }
  if (!flushed) return set_err(h, KSIM_E_DEVICE, "deferred-commit run ended without its flush");
  h->feed_past_end += launched - done;
  h->feed_odd_ends += (i - 1) & 1;
  return lazy_end_run(h, i - 1);
}

// ---- packed policy sweep (ksim_sweep_loaded; ksim_internal.h SweepLane) -------
// The lanes' buffers: one slab, carved at 256-byte steps (k_reset_copy moves
// 16-byte words), zero-filled; sized by (dc.n, lanes) and kept with the handle.
int alloc_sweep(ksim_handle* h, int32_t lanes) {
  if (int rc = sync_one_cut(h)) return rc;
  if (!h->sweep_tab)                                // its address is what the sweep graphs hold: allocated once
    if (const int rc = h->life_bufs.alloc(h, h->sweep_tab, sizeof(SweepLane) * kLazySlots * kSweepMaxLanes)) return rc;
  if (h->sweep_n == h->dc.n && lanes <= h->sweep_lanes) return KSIM_OK;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->sweep_slab.clear();
  h->sweep_n = -1;
  h->sweep_lanes = 0;
  h->sweep_lane.clear();
  const size_t n = (size_t)h->dc.n;
  size_t off = 0;
  auto take = [&](size_t bytes) {
    const size_t at = off;
    off += (bytes + 255) & ~(size_t)255;
    return at;
  };
  struct Off {
    size_t col[2][6], g, m, e, topk, cnt, cmp, pnorm, pinv;
  };
  std::vector<Off> offs((size_t)lanes);
  const size_t st_off = take(sizeof(DevState) * 2 * (size_t)lanes);
  for (auto& o : offs) {
    for (int p = 0; p < 2; p++)
      for (int k = 0; k < 6; k++) o.col[p][k] = take(k < 5 ? 8 * n : 4 * n);
    o.g = take(8 * (size_t)kLazySlots * kBatchPods);
    o.m = take(8 * (size_t)kLazySlots * kBatchPods);
    o.e = take(4 * (size_t)kLazySlots);
    o.topk = take(8 * (size_t)kBatchPods * kTopT);
    o.cnt = take(4 * (size_t)kBatchPods);
    o.cmp = take(4 * (size_t)kBatchPods);
    o.pnorm = take(8 * (size_t)kBatchPods * 4);
    o.pinv = take(4 * (size_t)kBatchPods);
  }
  char* base = nullptr;
  if (const int rc = h->sweep_slab.alloc(h, base, off)) return rc;
  h->sweep_st = (DevState*)(base + st_off);
  for (const auto& o : offs) {
    ksim_handle::SweepLaneBufs b{};
    for (int p = 0; p < 2; p++)
      b.x[p] = DynCols{(int64_t*)(base + o.col[p][0]), (int64_t*)(base + o.col[p][1]), (int64_t*)(base + o.col[p][2]),
                       (int64_t*)(base + o.col[p][3]), (int64_t*)(base + o.col[p][4]), (int32_t*)(base + o.col[p][5])};
    b.g = (uint64_t*)(base + o.g);
    b.m = (uint64_t*)(base + o.m);
    b.e = (int32_t*)(base + o.e);
    b.topk = (uint64_t*)(base + o.topk);
    b.topk_cnt = (int32_t*)(base + o.cnt);
    b.topk_complete = (int32_t*)(base + o.cmp);
    b.pnorm = (int64_t*)(base + o.pnorm);
    b.pinv = (int32_t*)(base + o.pinv);
    h->sweep_lane.push_back(b);
  }
  h->sweep_n = h->dc.n;
  h->sweep_lanes = lanes;
  return KSIM_OK;
}

// The table record of lane l at ring phase q (lazy_batch's arithmetic with
// the lane's buffers).
SweepLane sweep_record(const ksim_handle* h, int32_t l, int q, int32_t* row, const ksim_profile* prof,
                       const BatchProg* bp) {
  const ksim_handle::SweepLaneBufs& b = h->sweep_lane[(size_t)l];
  const int p = q & 1, q1 = (q + 3) & 3, q2 = (q + 2) & 3;
  DevState* st[2] = {h->sweep_st + 2 * (size_t)l, h->sweep_st + 2 * (size_t)l + 1};
  SweepLane r{};
  r.x_in = b.x[p ^ 1];
  r.step.w = b.x[p];
  r.step.st_in = st[p ^ 1];
  r.step.st_out = st[p];
  r.step.g1 = b.g + (size_t)q1 * kBatchPods;
  r.step.m1 = b.m + (size_t)q1 * kBatchPods;
  r.step.e1 = b.e + q1;
  r.step.g2 = b.g + (size_t)q2 * kBatchPods;
  r.step.e2 = b.e + q2;
  r.step.e_self = b.e + q;
  r.step.one_cut = h->one_cut ? 1 : 0;
  r.gkey = b.g + (size_t)q * kBatchPods;
  r.pmax = b.m + (size_t)q * kBatchPods;
  r.topk = b.topk;
  r.topk_cnt = b.topk_cnt;
  r.topk_complete = b.topk_complete;
  r.pnorm = b.pnorm;
  r.pinv = b.pinv;
  r.chosen = row;
  r.prof = prof;
  r.bp = bp;
  return r;
}

// Pods [a, b) under every vector, `lanes` vectors per launch (ksim_sweep_loaded
// has checked the conditions and uploaded the vectors' d_profs / d_bps).  The
// loop is run_lazy's with a lane dimension: every lane shares the batch index
// i (the ring phase and the column set), stretches are as long as the slowest
// live lane needs, each ends with a flush and one copy of the lanes' states.
// A lane that reached its end there hands out its row and state and takes the
// next pending vector: both column sets from the uploaded snapshot, both
// states zero with the run bounds, every ring slot empty, which is a valid
// start at any ring phase (lazy_begin).  A lane without a vector keeps cursor
// == end == 0 and empty slots: its blocks commit and evaluate nothing.
int run_sweep(ksim_handle* h, int32_t a, int32_t b, int32_t n_profs, int32_t lanes, bool def,
              const ksim_profile* d_profs, const BatchProg* d_bps, int32_t* chosen, ksim_batch_stats* stats) {
  int rc;
  if ((rc = alloc_sweep(h, lanes))) return rc;
  const int32_t np = h->dp.n_pods, count = b - a;
  if ((rc = h->sweep_rows.reserve(h, 4 * (size_t)lanes * (size_t)std::max(np, 1), Idle::kSync))) return rc;
  int32_t* rows = (int32_t*)h->sweep_rows.p;
  LaunchArgs la = make_args(h, h->dp, nullptr);
  const DevCluster c = la.c;
  const DevPods P = h->dp;                          // no static-class table: FAST runs do not read it
  SweepLane* const tab = h->sweep_tab;
  std::vector<SweepLane> htab((size_t)kLazySlots * kSweepMaxLanes);
  std::vector<int32_t> vec((size_t)lanes, -1), cur((size_t)lanes, 0);
  std::vector<DevState> hst(2 * (size_t)lanes);
  int32_t next_v = 0, live = 0;
  DevState st0[2] = {}, idle[2] = {};               // a lane's two states: at the run's start, without a vector
  st0[0].cursor = st0[1].cursor = a;
  st0[0].end = st0[1].end = b;
  auto arm = [&](int32_t l, int32_t v) -> int {     // v < 0: the lane idles
    const ksim_handle::SweepLaneBufs& B = h->sweep_lane[(size_t)l];
    HIPCHK(h, hipMemcpyAsync(h->sweep_st + 2 * (size_t)l, v >= 0 ? st0 : idle, 2 * sizeof(DevState),
                             hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemsetAsync(B.e, 0xff, 4 * kLazySlots, h->stream));
    if (v >= 0) {
      const size_t n = (size_t)h->dc.n;
      ResetList L;
      bool ok = true;
      for (int p = 0; p < 2; p++) {
        ok = ok && L.add(B.x[p].req_cpu, h->init.req_cpu, 8 * n) && L.add(B.x[p].req_mem, h->init.req_mem, 8 * n) &&
             L.add(B.x[p].req_eph, h->init.req_eph, 8 * n) && L.add(B.x[p].nz_cpu, h->init.nz_cpu, 8 * n) &&
             L.add(B.x[p].nz_mem, h->init.nz_mem, 8 * n) && L.add(B.x[p].num_pods, h->init.num_pods, 4 * n);
      }
      if (!ok) return set_err(h, KSIM_E_DEVICE, "packed sweep: snapshot columns not aligned for the reset copy");
      launch_reset_copy(L, h->stream);
      HIPCHK(h, hipGetLastError());
    }
    for (int q = 0; q < kLazySlots; q++)
      htab[(size_t)q * kSweepMaxLanes + l] =
          sweep_record(h, l, q, rows + (size_t)l * np, d_profs + std::max(v, 0), d_bps + std::max(v, 0));
    vec[(size_t)l] = v;
    cur[(size_t)l] = a;
    return KSIM_OK;
  };
  for (int32_t l = 0; l < lanes; l++) {
    const int32_t v = next_v < n_profs ? next_v++ : -1;
    if ((rc = arm(l, v))) return rc;
    live += v >= 0;
  }
  // st0 / idle / htab are read by the copies above when they are enqueued
  // (pageable memory: staged before hipMemcpyAsync returns)
  HIPCHK(h, hipMemcpyAsync(tab, htab.data(), sizeof(SweepLane) * htab.size(), hipMemcpyHostToDevice, h->stream));
  hipGraphExec_t graph;                             // captured by a run long enough to replay it
  if ((rc = handle_graph(h, {GraphKind::kSweep, {lanes, def}}, kGraphBatches, [&](int i) {
         launch_sweep_batch(c, P, tab + (size_t)(i & 3) * kSweepMaxLanes, lanes, def, h->stream);
       }, &graph, count >= kBatchPods * kGraphBatches)))
    return rc;
  auto phase_tab = [&](int64_t i) { return tab + (size_t)(i & 3) * kSweepMaxLanes; };
  int64_t i = 0;
  while (live > 0) {
    int32_t nb = 0;                                 // batches the slowest live lane still needs at most
    for (int32_t l = 0; l < lanes; l++)
      if (vec[(size_t)l] >= 0) nb = std::max(nb, (b - cur[(size_t)l] + kBatchPods - 1) / kBatchPods);
    const int32_t align = (int32_t)((kLazySlots - (i & 3)) & 3);
    // one graph per stretch at the most: the lanes are out of step, so some
    // lane nearly always has a long way to go, and a lane that ends inside a
    // long stretch would idle until its end instead of taking the next vector
    nb = std::min(nb, align + kGraphBatches);
    if (graph && nb >= align + kGraphBatches) {
      for (int32_t r = 0; r < align; r++, i++, nb--) launch_sweep_batch(c, P, phase_tab(i), lanes, def, h->stream);
      for (int32_t r = 0; r < nb / kGraphBatches; r++, i += kGraphBatches) HIPCHK(h, hipGraphLaunch(graph, h->stream));
    } else {
      for (int32_t r = 0; r < nb; r++, i++) launch_sweep_batch(c, P, phase_tab(i), lanes, def, h->stream);
    }
    launch_sweep_flush(c, P, phase_tab(i), lanes, h->stream);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(hst.data(), h->sweep_st, sizeof(DevState) * hst.size(), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    bool progress = false, retab = false;
    for (int32_t l = 0; l < lanes; l++) {
      const int32_t v = vec[(size_t)l];
      if (v < 0) continue;
      const DevState& st = hst[2 * (size_t)l + (size_t)(i & 1)];
      progress = progress || st.cursor > cur[(size_t)l];
      cur[(size_t)l] = st.cursor;
      if (st.cursor < b) continue;
      if (count)
        HIPCHK(h, hipMemcpyAsync(chosen + (size_t)v * count, rows + (size_t)l * np + a, 4 * (size_t)count,
                                 hipMemcpyDeviceToHost, h->stream));
      if (stats) {
        ksim_batch_stats& o = stats[v];
        o.pods = count;
        o.scheduled = st.scheduled;
        o.unschedulable = st.unschedulable;
        o.evals = st.evals;
        o.device_ms = 0;
        o.batches = st.batches;
        o.truncations = st.truncations;
        o.perpod_cycles = 0;
      }
      const int32_t nv = next_v < n_profs ? next_v++ : -1;
      if ((rc = arm(l, nv))) return rc;              // stream order: after the row's copy
      live -= nv < 0;
      retab = true;
    }
    if (!progress) return set_err(h, KSIM_E_DEVICE, "packed sweep made no progress");
    if (retab)
      HIPCHK(h, hipMemcpyAsync(tab, htab.data(), sizeof(SweepLane) * htab.size(), hipMemcpyHostToDevice, h->stream));
    i++;
  }
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return KSIM_OK;
}

int reset_counters(ksim_handle* h, hipStream_t stream);

// Run pods [a, b) on one path (all of them share the path: one of
// for_each_run's runs), in the form of its plan (plan_run on this handle).
int run_range(ksim_handle* h, int32_t a, int32_t b, const RunPlan& plan) {
  int rc;
  // No launch is ever issued past the end of the run (a launch there would
  // exit at once and skew per-kernel averages): whole graphs while they fit,
  // then single launches for the remainder.
  LaunchArgs la = make_args(h, h->dp, h->d_chosen);
  apply_plan(plan, la);
  // the call's counters are zeroed before its first run: by a deferred-commit
  // run's begin launch, which sets the run header too, or on their own
  const bool zero = h->counters_pending;
  h->counters_pending = false;
  if (plan.lazy()) return run_lazy(h, a, b, plan, la, zero);
  if (zero && (rc = reset_counters(h, h->stream))) return rc;
  if ((rc = set_run(h, a, b))) return rc;
  hipGraphExec_t graph;
  if (plan.form == RunForm::kPerPod) {
    const GraphKey key{GraphKind::kCycle, {plan.topo, la.fuse_min, la.fuse_ext, la.ptab}};
    if ((rc = handle_graph(h, key, kGraphCycles, [&](int) { launch_cycle(la, h->stream, false, plan.topo); }, &graph)))
      return rc;
    int32_t done = a;
    for (; done + kGraphCycles <= b; done += kGraphCycles) HIPCHK(h, hipGraphLaunch(graph, h->stream));
    for (; done < b; done++) launch_cycle(la, h->stream, false, plan.topo);
    HIPCHK(h, hipGetLastError());
    return KSIM_OK;
  }
  if (plan.form == RunForm::kTbatch) return run_tbatch(h, a, b, la);
  const auto one_batch = [&](int) { return plan.adapt() ? launch_batch_adapt(la, h->stream) : launch_batch(la, h->stream); };
  if ((rc = handle_graph(h, {GraphKind::kBatch, {la.fast, la.stab}}, kGraphBatches, one_batch, &graph))) return rc;
  // every batch commits between 1 and kBatchPods pods: a graph of
  // kGraphBatches batches never overshoots while left >= kBatchPods * kGraphBatches,
  // and ceil(left / kBatchPods) single batches never overshoot either
  int32_t cursor = a;
  while (cursor < b) {
    const int32_t left = b - cursor;
    if (left >= kBatchPods * kGraphBatches) {
      const int reps = left / (kBatchPods * kGraphBatches);
      for (int r = 0; r < reps; r++) HIPCHK(h, hipGraphLaunch(graph, h->stream));
    } else {
      const int n1 = (left + kBatchPods - 1) / kBatchPods;
      for (int r = 0; r < n1; r++) one_batch(r);
      HIPCHK(h, hipGetLastError());
    }
    DevState st;
    if ((rc = read_state(h, st))) return rc;
    if (st.cursor <= cursor) return set_err(h, KSIM_E_DEVICE, "batch path made no progress");
    cursor = st.cursor;
  }
  return KSIM_OK;
}

// Split [first, first+count) into maximal same-path runs (batch / per-pod,
// per-pod runs further by whether a pod carries topology uses).
// adapt_sharded: sharded handles whose shards follow adapt_shard_chunk, so
// ADAPT may take the sharded batch path (otherwise it runs cycle by cycle).
template <typename F>
int for_each_run(ksim_handle* h, int32_t first, int32_t count, F&& fn, bool adapt_sharded = false) {
  int32_t i = first;
  const int32_t end = first + count;
  while (i < end) {
    const bool batch_ok = !(adapt_mode(h) && is_sharded(h)) || adapt_sharded;
    const bool b = batch_ok && pod_on_batch(h, i);
    // a class-2 pod on the batch path with a use is an image pod (pod_batchable):
    // its one use is a static score part of its keys, not a topology input
    auto topo_of = [&](int32_t x) { return b && h->batchable[x] == 2 ? (uint8_t)0 : h->topo[x]; };
    const bool t = topo_of(i) != 0;
    int32_t j = i + 1;
    while (j < end && (batch_ok && pod_on_batch(h, j)) == b && topo_of(j) == topo_of(i)) j++;
    int rc = fn(i, j, b, t);
    if (rc) return rc;
    i = j;
  }
  return KSIM_OK;
}

// ---- node-sharded batch path ----------------------------------
// The shard-group runtime: five protocols (the P100 batch, the replicated
// deferred-commit batch, the replicated topology batch, the per-pod cycle, the
// ADAPT batch) over one exchange layer (group_all_gather, group_all_reduce),
// one graph cache (group_graph) and one run loop (group_run).
//
// A group is either {this rank's handle} with an RCCL communicator (one
// process per GPU) or an in-process group of shard handles on one device
// (exchanges by the group kernels).  Every member's kernels and the exchanges
// run on the leader's stream, asynchronously.
struct Group {
  const std::vector<ksim_handle*>& hs;
  ksim_handle* h0;                                // the leader: its stream, communicator and graph cache
  hipStream_t stream;
  int32_t world;
  explicit Group(const std::vector<ksim_handle*>& v)
      : hs(v), h0(v[0]), stream(v[0]->stream), world(v[0]->comm ? v[0]->world : (int32_t)v.size()) {}
  int32_t rank(size_t i) const { return h0->comm ? h0->rank : (int32_t)i; }
};

template <class F>
GroupPtrs group_ptrs(const Group& g, F&& ptr) {
  GroupPtrs p{};
  p.n = (int32_t)g.hs.size();
  for (size_t i = 0; i < g.hs.size(); i++) p.p[i] = (uint64_t*)ptr(g.hs[i]);
  return p;
}

// All-gather of `words` 8-byte words per member: src(h) -> dst(h) + rank * words.
// RCCL across processes, k_group_gather in process.
template <class S, class D>
int group_all_gather(const Group& g, S&& src, D&& dst, size_t words) {
  if (g.h0->comm) {
    const ncclResult_t r = rccl().all_gather(src(g.h0), dst(g.h0), words, ncclUint64, g.h0->comm, g.stream);
    if (r != ncclSuccess) return set_err(g.h0, KSIM_E_RCCL, std::string("ncclAllGather: ") + rccl().error_string(r));
    return KSIM_OK;
  }
  if (g.hs.size() * g.hs.size() * words > ((size_t)1 << 30))   // the kernel's grid stride counts in 32 bits
    return set_err(g.h0, KSIM_E_UNSUPPORTED, "shard group exchange too large for an in-process group");
  launch_group_gather(group_ptrs(g, src), group_ptrs(g, dst), (int32_t)words, g.stream);
  return KSIM_OK;
}

// Element-wise all-reduce of a per-member device buffer of `count` 8-byte
// words: sum (int64) or max (uint64).  RCCL across processes, k_group_reduce
// in process.
template <class F>
int group_all_reduce(const Group& g, F&& ptr, int64_t count, bool op_max) {
  if (count <= 0) return KSIM_OK;
  if (g.h0->comm) {
    void* b = (void*)ptr(g.h0);
    const ncclResult_t r = rccl().all_reduce(b, b, (size_t)count, op_max ? ncclUint64 : ncclInt64,
                                             op_max ? ncclMax : ncclSum, g.h0->comm, g.stream);
    if (r != ncclSuccess) return set_err(g.h0, KSIM_E_RCCL, std::string("ncclAllReduce: ") + rccl().error_string(r));
  } else if (g.hs.size() > 1) {
    launch_group_reduce(group_ptrs(g, ptr), count, op_max, g.stream);
  }
  return KSIM_OK;
}

constexpr auto sc_xsend = [](ksim_handle* h) { return h->sc.xsend; };
constexpr auto sc_xrecv = [](ksim_handle* h) { return h->sc.xrecv; };
constexpr auto sc_pmax = [](ksim_handle* h) { return h->sc.pmax; };

// reps x body(i) of one kind as a graph on the leader (its stream carries every
// member's kernels and the collectives), cached under `key` while the group is
// the same handles at the graph generations they had at capture; nullptr when
// capture is off or fails (the caller runs eagerly).
template <class B>
hipGraphExec_t group_graph(const Group& g, const GroupGraphKey& key, int reps, B&& body) {
  ksim_handle* h0 = g.h0;
  if (h0->sg_off || ab(kAbShardGraph)) return nullptr;
  std::vector<std::pair<const ksim_handle*, int64_t>> sig;
  for (auto* h : g.hs) sig.emplace_back(h, h->graph_gen);
  if (sig != h0->sg_sig) {                     // another group, or some handle dropped its graphs
    drop_group_graphs(h0);
    h0->sg_sig = sig;
  }
  auto it = h0->sg_graphs.find(key);
  if (it != h0->sg_graphs.end()) return it->second;
  if (hipStreamSynchronize(g.stream) != hipSuccess) return nullptr;
  hipGraphExec_t ge = nullptr;
  const char* what;
  const hipError_t e = capture_graph(g.stream, reps, body, &ge, what);
  (void)hipGetLastError();
  if (e != hipSuccess) {                       // e.g. a collective that cannot be captured
    h0->sg_off = true;
    h0->err.clear();
    return nullptr;
  }
  h0->graph_captures++;
  h0->sg_graphs.emplace(key, ge);
  return ge;
}

// The start of every group run: the run's range on every member, streams idle.
int group_begin(const Group& g, int32_t a, int32_t b) {
  for (auto* h : g.hs) {
    if (int rc = set_run(h, a, b)) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
  }
  return KSIM_OK;
}

// Pods [a, b) by stretches: enqueue(cursor) issues work that never passes the
// run's end, then the leader's state tells how far it got.
template <class E>
int group_run(const Group& g, int32_t a, int32_t b, const char* stuck, E&& enqueue) {
  if (int rc = group_begin(g, a, b)) return rc;
  int32_t cursor = a;
  while (cursor < b) {
    if (int rc = enqueue(cursor)) return rc;
    DevState st;
    HIPCHK(g.h0, hipMemcpyAsync(&st, g.h0->st, sizeof(st), hipMemcpyDeviceToHost, g.stream));
    HIPCHK(g.h0, hipStreamSynchronize(g.stream));
    if (st.cursor <= cursor) return set_err(g.h0, KSIM_E_DEVICE, stuck);
    cursor = st.cursor;
  }
  return KSIM_OK;
}

// group_run over batches that commit 1..kBatchPods pods each, so none is ever
// issued past the run's end: whole graphs of kGraphBatches batches while at
// least kBatchPods * kGraphBatches pods are left, then left / kBatchPods
// single batches.
template <class B>
int group_run_batches(const Group& g, int32_t a, int32_t b, const GroupGraphKey& key, const char* stuck, B&& batch) {
  hipGraphExec_t graph = nullptr;
  return group_run(g, a, b, stuck, [&](int32_t cursor) {
    const int32_t left = b - cursor;
    if (cursor == a && left >= kBatchPods * kGraphBatches)   // the first stretch: set_run done
      graph = group_graph(g, key, kGraphBatches, [&](int) { return batch(); });
    if (graph && left >= kBatchPods * kGraphBatches) {
      const int reps = left / (kBatchPods * kGraphBatches);
      for (int r = 0; r < reps; r++) HIPCHK(g.h0, hipGraphLaunch(graph, g.stream));
    } else {
      const int32_t n = std::max(1, left / kBatchPods);
      for (int32_t i = 0; i < n; i++)
        if (int rc = batch()) return rc;
    }
    return (int)KSIM_OK;
  });
}

// FAST keys for the run, on every shard of a group alike.
bool group_fast(const Group& g, int32_t a, int32_t b) {
  bool fast = run_fast(g.h0, a, b);
  for (auto* h : g.hs) fast = fast && h->alloc_narrow;
  return fast;
}

// Replicated handles hold every node: each evaluates its range (the only
// handles whose evaluation range is narrowed; ADAPT replicas run whole and
// never come here, so the ADAPT batch takes these arguments too).
LaunchArgs shard_args(ksim_handle* h, bool fast) {
  LaunchArgs la = make_args(h, h->dp, h->d_chosen);
  la.fast = fast;
  if (h->replicated) {
    la.c.eval_lo = h->eval_lo;
    la.c.eval_hi = h->eval_hi;
  }
  return la;
}

// One batch on every shard of a group, phases separated by the two exchanges:
// all-gather of the per-shard candidate records, all-reduce (max) of the pair
// keys.  On replicated handles the pair keys and binds of every guess are
// local, so the pair-key all-reduce is not needed (one exchange per batch).
int shard_batch(const Group& g, bool fast) {
  int rc;
  for (auto* h : g.hs) launch_shard_eval(shard_args(h, fast), g.stream);
  if ((rc = group_all_gather(g, sc_xsend, sc_xrecv, (size_t)kBatchPods * kXRec))) return rc;
  for (auto* h : g.hs) launch_shard_chain(shard_args(h, fast), g.world, g.stream);
  if (!g.h0->replicated && (rc = group_all_reduce(g, sc_pmax, kBatchPods, true))) return rc;
  for (auto* h : g.hs) launch_shard_commit(shard_args(h, fast), g.stream);
  HIPCHK(g.h0, hipGetLastError());
  return KSIM_OK;
}

// ---- replicated deferred-commit batches (ksim_internal.h) -----------------------
// Replicated handles of a FAST P100 run: batch i is k_batch_top_commit over the
// replica's node range (the commit of batch i-1 included, every replica binds
// every placement), the records' all-gather, the global merge and the chain +
// pairs: one exchange and three launches per batch instead of four.
bool lazy_rep_ok(const Group& g, int32_t a, int32_t b, bool fast) {
  if (!fast || !lazy_enabled()) return false;
  for (auto* h : g.hs) {
    if (!h->replicated || h->dc.base != 0 || h->dc.n > kLazyMaxNodes || h->dc.n <= 0) return false;
    for (int32_t i = a; i < b; i++)
      if (!h->noadd[i]) return false;
  }
  return true;
}

int shard_batch_lazy(const Group& g, int64_t i) {
  for (auto* h : g.hs) launch_lazy_top_rep(lazy_batch(h, shard_args(h, true), i), h->sc.xsend, g.stream);
  if (int rc = group_all_gather(g, sc_xsend, sc_xrecv, (size_t)kBatchPods * kXRec)) return rc;
  for (auto* h : g.hs) launch_lazy_chain_rep(lazy_batch(h, shard_args(h, true), i), g.world, g.stream);
  HIPCHK(g.h0, hipGetLastError());
  return KSIM_OK;
}

// As run_lazy, on the group's stream.  The ring alignment of the graph and the
// parity of the state read are this loop's own (not group_run's).
int shard_run_lazy(const Group& g, int32_t a, int32_t b) {
  ksim_handle* h0 = g.h0;
  hipStream_t stream = g.stream;
  int rc;
  if ((rc = group_begin(g, a, b))) return rc;
  for (auto* h : g.hs) {
    if ((rc = lazy_begin(h))) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
  }
  GroupGraphKey key{};
  key.kind = GroupGraphKind::kLazyBatch;
  const hipGraphExec_t graph =
      b - a >= kBatchPods * kGraphBatches
          ? group_graph(g, key, kGraphBatches, [&](int i) { return shard_batch_lazy(g, i); })
          : nullptr;
  int64_t i = 0;
  int32_t cursor = a;
  while (cursor < b) {
    int32_t nb = (b - cursor + kBatchPods - 1) / kBatchPods;
    const int32_t align = (int32_t)((kLazySlots - (i & 3)) & 3);
    if (graph && nb >= align + kGraphBatches) {
      for (int32_t r = 0; r < align; r++, i++, nb--)
        if ((rc = shard_batch_lazy(g, i))) return rc;
      for (int32_t r = 0; r < nb / kGraphBatches; r++, i += kGraphBatches) HIPCHK(h0, hipGraphLaunch(graph, stream));
    } else {
      for (int32_t r = 0; r < nb; r++, i++)
        if ((rc = shard_batch_lazy(g, i))) return rc;
    }
    for (auto* h : g.hs) launch_lazy_flush(lazy_batch(h, shard_args(h, true), i), stream);
    HIPCHK(h0, hipGetLastError());
    DevState st;
    HIPCHK(h0, hipMemcpyAsync(&st, (i & 1) ? h0->lazy.st1 : h0->st, sizeof(st), hipMemcpyDeviceToHost, stream));
    HIPCHK(h0, hipStreamSynchronize(stream));
    if (st.cursor <= cursor) return set_err(h0, KSIM_E_DEVICE, "replicated deferred-commit batches made no progress");
    cursor = st.cursor;
    i++;
  }
  for (auto* h : g.hs) {
    if ((rc = lazy_end(h, i - 1))) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
  }
  return KSIM_OK;
}

// Pods [a, b) on the sharded batch path (every pod must be batchable).
int shard_run(const Group& g, int32_t a, int32_t b) {
  const bool fast = group_fast(g, a, b);
  if (lazy_rep_ok(g, a, b, fast)) return shard_run_lazy(g, a, b);
  GroupGraphKey key{};
  key.kind = GroupGraphKind::kBatch;
  key.fast = fast;
  return group_run_batches(g, a, b, key, "sharded batch path made no progress", [&] { return shard_batch(g, fast); });
}

// ---- replicated topology batches (ksim_tbatch.hip launch_tb_rep_*) -------------
// One topology batch on every replica of a group: each evaluates its node
// range; three exchanges (the filter's per-pod counters and extrema, the
// per-pod top-T records with the extremum holder counts, the pair maxima and
// pinv); every replica commits every placement.
int shard_tbatch(const Group& g) {
  static_assert(sizeof(WinState) % 8 == 0, "the window states are exchanged in 8-byte words");
  int rc;
  for (auto* h : g.hs) launch_tb_rep_filter(shard_args(h, false), g.stream);
  if ((rc = group_all_gather(g, [](ksim_handle* h) { return h->sc.tb_win; },
                             [](ksim_handle* h) { return h->sc.tb_xrecv; }, sizeof(WinState) / 8 * kTbPods)))
    return rc;
  for (auto* h : g.hs) launch_tb_rep_select(shard_args(h, false), g.world, g.stream);
  if ((rc = group_all_gather(g, sc_xsend, sc_xrecv, (size_t)kTbPods * kTbXRec))) return rc;
  for (auto* h : g.hs) launch_tb_rep_pairs(shard_args(h, false), g.world, g.stream);
  if ((rc = group_all_reduce(g, [](ksim_handle* h) { return h->sc.tb_pp; }, 2 * kTbPods, true))) return rc;
  for (auto* h : g.hs) launch_tb_rep_commit(shard_args(h, false), g.stream);
  HIPCHK(g.h0, hipGetLastError());
  return KSIM_OK;
}

// Topology batch pods [a, b) on the replicas of a group (as run_tbatch: the
// batches the run lengths predict, then the state).
int shard_run_tbatch(const Group& g, int32_t a, int32_t b) {
  for (auto* h : g.hs) HIPCHK(h, hipMemsetAsync(h->sc.tb_win, 0, sizeof(WinState) * kTbPods, h->stream));
  return group_run(g, a, b, "replicated topology batches made no progress", [&](int32_t cursor) {
    int32_t nbat = 0;
    for (int32_t i = cursor; i < b; nbat++) i += std::min(std::min(kTbPods, b - i), std::max(g.h0->tlen_plain[i], 1));
    for (int32_t i = 0; i < nbat; i++)
      if (int rc = shard_tbatch(g)) return rc;
    return (int)KSIM_OK;
  });
}

// ---- node-sharded per-pod cycle (C1 extrema, C2 argmax, C3 window) ----
// One per-pod cycle (the pod at the shards' common cursor) across node shards,
// with exchanges of xdom / xreg words (at least the pod's own lengths: words
// past them are summed but never read).  The two-word all-gathers:
// s.xsend[0..1] -> s.xrecv[world][2].
int shard_cycle(const Group& g, bool topo, int64_t xdom, int64_t xreg) {
  hipStream_t stream = g.stream;
  int rc;
  if (topo) {
    for (auto* h : g.hs) launch_pshard_topo(make_args(h, h->dp, h->d_chosen), stream);
    if ((rc = group_all_reduce(g, [](ksim_handle* h) { return h->sc.xdom; }, xdom, false))) return rc;
  }
  for (auto* h : g.hs) launch_pshard_filter(make_args(h, h->dp, h->d_chosen), topo, stream);
  if ((rc = group_all_gather(g, sc_xsend, sc_xrecv, 2))) return rc;      // C3: feasible counts per shard
  for (size_t i = 0; i < g.hs.size(); i++)
    launch_pshard_window(make_args(g.hs[i], g.hs[i]->dp, g.hs[i]->d_chosen), g.rank(i), g.world, stream);
  if ((rc = group_all_reduce(g, [](ksim_handle* h) { return h->sc.xreg; }, xreg, false))) return rc;
  for (auto* h : g.hs) launch_pshard_extrema(make_args(h, h->dp, h->d_chosen), xreg > 0, stream);
  if ((rc = group_all_reduce(g, [](ksim_handle* h) { return h->sc.win->ext; }, kExtWords, true))) return rc;
  for (auto* h : g.hs) launch_pshard_select(make_args(h, h->dp, h->d_chosen), stream);
  if ((rc = group_all_gather(g, sc_xsend, sc_xrecv, 2))) return rc;      // C2: every shard's (total, TB) best
  for (auto* h : g.hs) launch_pshard_bind(make_args(h, h->dp, h->d_chosen), g.world, stream);
  HIPCHK(g.h0, hipGetLastError());
  return KSIM_OK;
}

// Pods [a, b) on the sharded per-pod path, one cycle each: whole graphs of
// kGraphCycles cycles shaped for the run's largest exchanges, then single
// cycles for the rest.
int shard_run_perpod(const Group& g, int32_t a, int32_t b) {
  const ksim_handle* h0 = g.h0;
  if (int rc = group_begin(g, a, b)) return rc;
  int32_t i = a;
  if (b - a >= kGraphCycles) {
    GroupGraphKey key{};
    key.kind = GroupGraphKind::kPerPod;
    key.topo = h0->topo[a] != 0;                 // runs are uniform in topo (for_each_run)
    for (int32_t k = a; k < b; k++) {
      key.xdom = std::max(key.xdom, h0->xdom_len[k]);
      key.xreg = std::max(key.xreg, h0->xreg_len[k]);
    }
    if (hipGraphExec_t graph = group_graph(g, key, kGraphCycles,
                                           [&](int) { return shard_cycle(g, key.topo, key.xdom, key.xreg); }))
      for (; i + kGraphCycles <= b; i += kGraphCycles) HIPCHK(g.h0, hipGraphLaunch(graph, g.stream));
  }
  for (; i < b; i++)
    if (int rc = shard_cycle(g, h0->topo[i] != 0, h0->xdom_len[i], h0->xreg_len[i])) return rc;
  return KSIM_OK;
}

// ---- node-sharded ADAPT batch path (ksim_adapt.hip "node-sharded ADAPT batch") ----
// The shard layout it needs: R shards of chunk = ceil(ceil(N / R) / 64) * 64
// nodes each (the last one the rest, non-empty), in order (ksim/shard.py
// partition follows it whenever it can).
int32_t adapt_shard_chunk(int32_t n_total, int32_t world) {
  const int32_t q = (n_total + world - 1) / world;
  return (q + 63) / 64 * 64;
}

bool adapt_shard_layout(const Group& g) {
  const int32_t N = g.h0->dc.n_total, chunk = adapt_shard_chunk(N, g.world);
  if ((int64_t)(g.world - 1) * chunk >= N) return false;
  for (size_t i = 0; i < g.hs.size(); i++) {
    const int32_t base = g.rank(i) * chunk, n = std::min(chunk, N - base);
    if (g.hs[i]->dc.base != base || g.hs[i]->dc.n != n) return false;
  }
  return true;
}

int adapt_shard_buffers(ksim_handle* h, int32_t world, int32_t W) {
  if (h->ash.world == world && h->ash.w == W) return KSIM_OK;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  drop_cycle_graphs(h);                           // shard batch graphs captured over the old buffers
  h->ash = AshBufs{};
  const size_t nw = (size_t)(h->dc.n_total + 63) / 64;
  int rc;
  if ((rc = h->ash.bufs.alloc(h, h->ash.send, 8 * (size_t)kBatchPods * W)) ||
      (rc = h->ash.bufs.alloc(h, h->ash.recv, 8 * (size_t)world * kBatchPods * W)) ||
      (rc = h->ash.bufs.alloc(h, h->ash.gmask, 8 * (size_t)kBatchPods * nw)))
    return rc;
  h->ash.world = world;
  h->ash.w = W;
  return KSIM_OK;
}

// One ADAPT batch on every shard of a group (exchanges: bitmaps of W words per
// pod, records, M).
int shard_batch_adapt(const Group& g, int32_t W, bool fast) {
  int rc;
  for (auto* h : g.hs) launch_adapt_sh_mask(shard_args(h, fast), h->ash.send, W, g.stream);
  if ((rc = group_all_gather(g, [](ksim_handle* h) { return h->ash.send; },
                             [](ksim_handle* h) { return h->ash.recv; }, (size_t)kBatchPods * W)))
    return rc;
  for (auto* h : g.hs) launch_adapt_sh_window(shard_args(h, fast), h->ash.recv, W, h->ash.gmask, g.stream);
  if ((rc = group_all_gather(g, sc_xsend, sc_xrecv, (size_t)kBatchPods * kXRec))) return rc;
  for (auto* h : g.hs) launch_adapt_sh_pairs(shard_args(h, fast), h->ash.gmask, g.world, g.stream);
  if ((rc = group_all_reduce(g, sc_pmax, 2 * kBatchPods, true))) return rc;
  for (auto* h : g.hs) launch_adapt_sh_commit(shard_args(h, fast), g.stream);
  HIPCHK(g.h0, hipGetLastError());
  return KSIM_OK;
}

// Pods [a, b) on the sharded ADAPT batch path.
int shard_run_adapt(const Group& g, int32_t a, int32_t b) {
  const int32_t W = adapt_shard_chunk(g.h0->dc.n_total, g.world) / 64;
  const bool fast = group_fast(g, a, b);
  for (auto* h : g.hs)
    if (int rc = adapt_shard_buffers(h, g.world, W)) return rc;
  GroupGraphKey key{};
  key.kind = GroupGraphKind::kAdaptBatch;
  key.fast = fast;
  return group_run_batches(g, a, b, key, "sharded ADAPT batch path made no progress",
                           [&] { return shard_batch_adapt(g, W, fast); });
}

// A sharded run: batchable stretches on the batch protocol, the rest cycle by cycle.
int shard_schedule(const std::vector<ksim_handle*>& hs, int32_t first, int32_t count) {
  const Group g(hs);
  if (profile_nb(g.h0->prof))
    return set_err(g.h0, KSIM_E_UNSUPPORTED, "NetworkBandwidth profiles run on unsharded handles");
  const bool adapt = adapt_mode(g.h0);
  if (g.h0->replicated) {
    // P100 batch stretches on the replicated exchange; everything else runs
    // whole on every replica (the same cycles, so the replicas stay equal)
    return for_each_run(g.h0, first, count, [&](int32_t a, int32_t b, bool batch, bool topo) {
      if (batch && !adapt) return topo ? shard_run_tbatch(g, a, b) : shard_run(g, a, b);
      for (auto* h : hs) {
        if (int rc = run_range(h, a, b, plan_run(h, a, b, batch, topo))) return rc;
      }
      return (int)KSIM_OK;
    }, true);
  }
  const bool adapt_batch = adapt && adapt_shard_layout(g);
  return for_each_run(g.h0, first, count, [&](int32_t a, int32_t b, bool batch, bool) {
    if (!batch) return shard_run_perpod(g, a, b);
    return adapt ? shard_run_adapt(g, a, b) : shard_run(g, a, b);
  }, adapt_batch);
}

int reset_counters(ksim_handle* h, hipStream_t stream) {
  HIPCHK(h, hipMemsetAsync(&h->st->truncations, 0, 4, stream));
  HIPCHK(h, hipMemsetAsync(&h->st->evals, 0, 3 * sizeof(int64_t), stream));
  HIPCHK(h, hipMemsetAsync(&h->st->batches, 0, 4, stream));
  HIPCHK(h, hipMemsetAsync(&h->st->cuts, 0, 8, stream));
  static_assert(offsetof(DevState, stretch_pods) == offsetof(DevState, stretches) + 4, "the stretch counters are adjacent");
  HIPCHK(h, hipMemsetAsync(&h->st->stretches, 0, 8, stream));
  return KSIM_OK;
}

}  // namespace

int ksim_abi_version(void) { return KSIM_ABI_VERSION; }

size_t ksim_abi_sizeof(int which) {
  switch (which) {
    case 0: return sizeof(ksim_node_table);
    case 1: return sizeof(ksim_vocab);
    case 2: return sizeof(ksim_label_expr);
    case 3: return sizeof(ksim_term);
    case 4: return sizeof(ksim_pod);
    case 5: return sizeof(ksim_pod_set);
    case 6: return sizeof(ksim_profile);
    case 7: return sizeof(ksim_eval_out);
    case 8: return sizeof(ksim_batch_stats);
    case 9: return sizeof(ksim_topo_use);
    case 10: return sizeof(ksim_class_add);
    case 11: return sizeof(ksim_match_problem);
    case 12: return sizeof(ksim_k8s_kv);
    case 13: return sizeof(ksim_k8s_taint);
    case 14: return sizeof(ksim_k8s_toleration);
    case 15: return sizeof(ksim_k8s_requirement);
    case 16: return sizeof(ksim_k8s_selector_term);
    case 17: return sizeof(ksim_k8s_preferred_term);
    case 18: return sizeof(ksim_k8s_label_selector);
    case 19: return sizeof(ksim_k8s_pod_term);
    case 20: return sizeof(ksim_k8s_spread);
    case 21: return sizeof(ksim_k8s_port);
    case 22: return sizeof(ksim_k8s_container);
    case 23: return sizeof(ksim_k8s_image);
    case 24: return sizeof(ksim_k8s_volume_group);
    case 25: return sizeof(ksim_k8s_node);
    case 26: return sizeof(ksim_k8s_pod);
    case 27: return sizeof(ksim_k8s_namespace);
    case 28: return sizeof(ksim_k8s_service);
    case 29: return sizeof(ksim_k8s_controller);
    case 30: return sizeof(ksim_k8s_pool);
    case 31: return sizeof(ksim_encode_nodes_opts);
    case 32: return sizeof(ksim_encode_pods_opts);
    case 33: return sizeof(ksim_encoder_info);
    default: return 0;
  }
}

int ksim_create(int device, ksim_handle** out) {
  if (!out) return KSIM_E_INVALID;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return KSIM_E_DEVICE;
  if (device < 0 || device >= ndev) return KSIM_E_INVALID;
  if (hipSetDevice(device) != hipSuccess) return KSIM_E_DEVICE;
  auto* h = new ksim_handle();
  h->device = device;
  // d_prof / d_bp are written only by ksim_set_profile, on the engine's stream
  // (like the zero fill here); st is zero before any stream reads it
  if (hipStreamCreateWithFlags(h->stream.out(), hipStreamNonBlocking) != hipSuccess ||
      hipEventCreate(h->ev0.out()) != hipSuccess || hipEventCreate(h->ev1.out()) != hipSuccess ||
      h->life_bufs.alloc(h, h->st, sizeof(DevState)) || h->life_bufs.alloc(h, h->d_prof, sizeof(ksim_profile)) ||
      h->life_bufs.alloc(h, h->d_bp, sizeof(BatchProg)) || hipStreamSynchronize(h->stream) != hipSuccess) {
    delete h;                                      // on its device (set above): releases what was made
    return KSIM_E_DEVICE;
  }
  *out = h;
  return KSIM_OK;
}

// Everything the handle owns goes in its members' destructors (ksim_mem.h), on
// the handle's device, the stream drained first.
void ksim_destroy(ksim_handle* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  drop_graphs(h);
  if (h->comm && rccl().ok) (void)rccl().comm_destroy(h->comm);
  delete h;
}

const char* ksim_last_error(const ksim_handle* h) { return h ? h->err.c_str() : "null handle"; }

// What ksim_set_profile accepts (ksim_sweep_loaded checks every vector the same way).
static int validate_profile(ksim_handle* h, const ksim_profile* p) {
  if (p->n_filter < 0 || p->n_filter > KSIM_MAX_FILTER || p->n_score < 0 || p->n_score > KSIM_MAX_SCORE)
    return set_err(h, KSIM_E_INVALID, "plugin count out of range");
  for (int i = 0; i < p->n_filter; i++) {
    if (!plugin_supported(p->filter[i])) return set_err(h, KSIM_E_INVALID, "unknown filter plugin id");
    for (int j = 0; j < i; j++)
      if (p->filter[j] == p->filter[i]) return set_err(h, KSIM_E_INVALID, "filter plugin listed twice");
  }
  for (int i = 0; i < p->n_score; i++) {
    if (!plugin_supported(p->score[i])) return set_err(h, KSIM_E_INVALID, "unknown score plugin id");
    for (int j = 0; j < i; j++)
      if (p->score[j] == p->score[i]) return set_err(h, KSIM_E_INVALID, "score plugin listed twice");
    if (p->score_weight[i] < 0) return set_err(h, KSIM_E_INVALID, "negative score weight");
  }
  if (p->fit_n_res < 0 || p->fit_n_res > KSIM_MAX_RES || p->ba_n_res < 0 || p->ba_n_res > KSIM_MAX_RES)
    return set_err(h, KSIM_E_INVALID, "scoring resources out of range");
  // NodeResourcesFitArgs / DefaultPreemptionArgs as validation.ValidateNodeResourcesFitArgs /
  // ValidateDefaultPreemptionArgs accept them (the plugin constructors refuse anything else)
  if (p->fit_strategy < KSIM_FIT_LEAST_ALLOCATED || p->fit_strategy > KSIM_FIT_REQUESTED_TO_CAPACITY_RATIO)
    return set_err(h, KSIM_E_INVALID, "unknown NodeResourcesFit scoring strategy");
  if (p->fit_strategy == KSIM_FIT_REQUESTED_TO_CAPACITY_RATIO) {
    if (p->fit_n_shape < 1 || p->fit_n_shape > KSIM_MAX_SHAPE)
      return set_err(h, KSIM_E_INVALID, "RequestedToCapacityRatio shape: 1..16 points");
    for (int i = 0; i < p->fit_n_shape; i++) {
      if (p->fit_shape_util[i] < 0 || p->fit_shape_util[i] > 100 || (i > 0 && p->fit_shape_util[i] <= p->fit_shape_util[i - 1]))
        return set_err(h, KSIM_E_INVALID, "RequestedToCapacityRatio shape: utilization strictly increasing in [0, 100]");
      if (p->fit_shape_score[i] < 0 || p->fit_shape_score[i] > 100 || p->fit_shape_score[i] % 10 != 0)
        return set_err(h, KSIM_E_INVALID, "RequestedToCapacityRatio shape: score x 10 in [0, 100]");
    }
  }
  if (p->fit_ignored_scalar >> KSIM_MAX_SCALAR) return set_err(h, KSIM_E_INVALID, "fit_ignored_scalar past the scalar columns");
  if (p->preempt_min_pct < 0 || p->preempt_min_pct > 100 || p->preempt_min_abs < 0 ||
      (p->preempt_min_pct == 0 && p->preempt_min_abs == 0))
    return set_err(h, KSIM_E_INVALID, "DefaultPreemptionArgs: minCandidateNodesPercentage in [0, 100], "
                                      "minCandidateNodesAbsolute >= 0, not both 0");
  return KSIM_OK;
}

// The profile compiled for batchable pods (see BatchProg in ksim_device.h).
static BatchProg compile_batch_prog(const ksim_profile* p) {
  BatchProg bp{};
  // the FAST / cpu-memory keys implement LeastAllocated; the other strategies
  // take the generic keys (fit_score)
  bp.cpu_mem = p->fit_strategy == KSIM_FIT_LEAST_ALLOCATED && p->fit_n_res == 2 && p->fit_res[0] == KSIM_RES_CPU &&
               p->fit_res[1] == KSIM_RES_MEMORY && p->ba_n_res == 2 && p->ba_res[0] == KSIM_RES_CPU &&
               p->ba_res[1] == KSIM_RES_MEMORY;
  bp.fit_w_cpu = p->fit_res_weight[0];
  bp.fit_w_mem = p->fit_res_weight[1];
  bp.fast_w = bp.cpu_mem && bp.fit_w_cpu >= 1 && bp.fit_w_cpu < (1ll << 31) && bp.fit_w_mem >= 1 &&
              bp.fit_w_mem < (1ll << 31);
  bp.no_score = p->n_score == 0;
  bp.fit_w_eq = bp.fast_w && bp.fit_w_cpu == bp.fit_w_mem;
  if (bp.fast_w) {                                    // RN(1 / w): IEEE division on the host
    bp.inv_w[0] = 1.0 / (double)bp.fit_w_cpu;
    bp.inv_w[1] = 1.0 / (double)bp.fit_w_mem;
    bp.inv_w[2] = 1.0 / (double)(bp.fit_w_cpu + bp.fit_w_mem);
  }
  for (int i = 0; i < p->n_filter; i++) {
    const int f = p->filter[i];
    if (f == KSIM_PL_NODE_UNSCHEDULABLE || f == KSIM_PL_NODE_NAME || f == KSIM_PL_TAINT_TOLERATION ||
        f == KSIM_PL_NODE_AFFINITY)
      bp.static_filter[bp.n_static++] = (uint8_t)f;
    if (f == KSIM_PL_NODE_RESOURCES_FIT) bp.has_fit_filter = 1;
  }
  for (int k = 0; k < p->n_score; k++) {
    const int64_t w = p->score_weight[k] == 0 ? 1 : p->score_weight[k];
    if (p->score[k] == KSIM_PL_NODE_RESOURCES_FIT) bp.w_fit += w;
    if (p->score[k] == KSIM_PL_BALANCED_ALLOCATION) bp.w_ba += w;
    if (p->score[k] == KSIM_PL_TAINT_TOLERATION) bp.w_tt += w;
    if (p->score[k] == KSIM_PL_NODE_AFFINITY) bp.w_na += w;
    if (p->score[k] == KSIM_PL_IMAGE_LOCALITY) bp.w_il += w;
  }
  plan_profile(*p, bp.rank_lo, bp.rank_hi, bp.slot, bp.slot_hi);
  return bp;
}

int ksim_set_profile(ksim_handle* h, const ksim_profile* p) {
  if (const int prc = flush_pend_bind(h)) return prc;   // a queued Reserve lands first
  if (!h || !p) return KSIM_E_INVALID;
  h->stab_dirty = true;                     // DevPods::stab: the static filter list may change
  if (const int vrc = validate_profile(h, p)) return vrc;
  const BatchProg bp = compile_batch_prog(p);
  HIPCHK(h, hipSetDevice(h->device));
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  // the batch graphs read the profile from d_prof / d_bp; only the ADAPT
  // window size K is captured by value (from percentageOfNodesToScore)
  // and the Fit filter's ignored scalar columns (DevCluster::fit_ignore); the
  // launch picks the evaluation kernel by the FAST key's shape (fast_def)
  const bool keep_batch_graphs = h->has_profile &&
                                 h->prof.percentage_of_nodes_to_score == p->percentage_of_nodes_to_score &&
                                 h->dc.fit_ignore == p->fit_ignored_scalar && fast_def(h->bp) == fast_def(bp);
  // batchability depends on the profile: a loaded queue must be reloaded (its
  // buffers stay allocated for ksim_load_pods to reuse)
  h->dp = DevPods{};
  h->batchable.clear();
  // device copies first: if one fails the handle holds no profile at all (never
  // a host profile the device copies and the kept graphs disagree with)
  hipError_t e = hipMemcpyAsync(h->d_prof, p, sizeof(ksim_profile), hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(h->d_bp, &bp, sizeof(BatchProg), hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess) {
    drop_graphs(h);
    h->has_profile = false;
    return hip_fail(h, e, "profile upload");
  }
  h->prof = *p;
  h->bp = bp;
  h->dc.fit_ignore = p->fit_ignored_scalar;
  h->has_profile = true;
  if (keep_batch_graphs)
    drop_cycle_graphs(h);
  else
    drop_graphs(h);
  return KSIM_OK;
}

// Device copies of topology uses carry kUseUniqueCol when their key column is
// unique per node (ksim_device.h use_node_count).
// A KSIM_USE_VOLUME copy carries its family in _pad and no column, so nothing
// that walks a pod's uses reads a label column for it.
static void mark_unique(const ksim_handle* h, ksim_topo_use* u, size_t n) {
  for (size_t i = 0; i < n; i++)
    if (u[i].kind == KSIM_USE_VOLUME) {
      if (u[i].col == KSIM_COL_NONE) continue;   // a copy already (validate_pod admits no such family)
      u[i]._pad = u[i].col;
      u[i].col = KSIM_COL_NONE;
    } else if (u[i].col != KSIM_COL_NONE && u[i].col < h->col_unique.size() && h->col_unique[u[i].col])
      u[i].flags |= kUseUniqueCol;
}

// The pod's PodPlan against the current profile and cluster (uses: its device
// copies, kUseUniqueCol marked).
static PodPlan make_plan(const ksim_handle* h, const ksim_pod& p, const ksim_topo_use* uses) {
  PodPlan pl{};
  pl.m = use_masks(h->prof, uses, p.use_count);
  pl.filter_en = plan_filter_en(h->prof, p, pl.m, h->any_unschedulable, !h->hard_taints.empty());
  return pl;
}

// Re-based copy of one pod with only the expressions/terms it references.
static void single_pod_set(const ksim_pod_set* ps, int32_t i, ksim_pod& pod, std::vector<ksim_label_expr>& ex,
                           std::vector<ksim_term>& tm, std::vector<ksim_topo_use>& us,
                           std::vector<ksim_class_add>& ad, std::vector<int32_t>& nn) {
  pod = ps->pods[i];
  us.assign(ps->uses + pod.use_first, ps->uses + pod.use_first + pod.use_count);
  ad.assign(ps->adds + pod.add_first, ps->adds + pod.add_first + pod.add_count);
  if ((pod.flags & KSIM_POD_NODE_NAMES) && pod.nn_count > 0)
    nn.assign(ps->nn + pod.nn_first, ps->nn + pod.nn_first + pod.nn_count);
  pod.use_first = 0;
  pod.add_first = 0;
  pod.nn_first = 0;
  int32_t sel0 = (int32_t)ex.size();
  for (int32_t k = 0; k < pod.sel_count; k++) ex.push_back(ps->exprs[pod.sel_first + k]);
  pod.sel_first = sel0;
  auto copy_terms = [&](int32_t& first, int32_t count) {
    int32_t t0 = (int32_t)tm.size();
    for (int32_t t = 0; t < count; t++) {
      ksim_term x = ps->terms[first + t];
      int32_t e0 = (int32_t)ex.size();
      for (int32_t k = 0; k < x.n_expr; k++) ex.push_back(ps->exprs[x.first_expr + k]);
      x.first_expr = e0;
      tm.push_back(x);
    }
    first = t0;
  };
  copy_terms(pod.req_term_first, pod.req_term_count);
  copy_terms(pod.pref_term_first, pod.pref_term_count);
  copy_terms(pod.added_term_first, pod.added_term_count);
  copy_terms(pod.vb_first, pod.vb_count);
  copy_terms(pod.vz_first, pod.vz_count);
}

// Copies to / from the pinned staging by one kernel (launch_copy_list).
struct Copies {
  CopyList l{};
  int n = 0;
  Copies() { l.anode = -1; }
  void add(const void* src, void* dst, size_t bytes) {
    if (!bytes) return;
    l.src[n] = (const uint8_t*)src;
    l.dst[n] = (uint8_t*)dst;
    l.n[n] = (uint32_t)bytes;
    n++;
  }
  // a framework-driven filter pass's start in the same launch (launch_fw_begin)
  void begin(DevState* st, WinState* win, int32_t first, int32_t end) {
    l.bst = st;
    l.bwin = win;
    l.bfirst = first;
    l.bend = end;
  }
  // a queued bind in the same launch
  void bind(const DevCluster& c, const DevPods& P, int32_t node, int sign) {
    l.ac = c;
    l.aP = P;
    l.anode = node;
    l.asign = sign;
  }
  int run(ksim_handle* h) {
    if (n || l.bst || l.anode >= 0) launch_copy_list(l, n, h->stream);
    HIPCHK(h, hipGetLastError());
    return KSIM_OK;
  }
};

static void build_pod_blob(ksim_handle* h, const ksim_pod_set* ps, int32_t pod_index, PodBlob& b) {
  ksim_pod pod;
  std::vector<ksim_label_expr>& ex = h->bs_ex;
  std::vector<ksim_term>& tm = h->bs_tm;
  std::vector<ksim_topo_use>& us = h->bs_us;
  std::vector<ksim_class_add>& ad = h->bs_ad;
  std::vector<int32_t>& nn = h->bs_nn;
  ex.clear();                              // single_pod_set appends
  tm.clear();
  nn.clear();
  single_pod_set(ps, pod_index, pod, ex, tm, us, ad, nn);
  mark_unique(h, us.data(), us.size());
  int32_t bflag[4] = {0, 0, 0, 0};
  for (const auto& u : us)
    if (use_registers_values(u)) bflag[0] |= kPodRegistersValues;
  const PodPlan plan = make_plan(h, pod, us.data());
  struct Piece {
    const void* src;
    size_t bytes;
  };
  const Piece pc[8] = {{&pod, sizeof(pod)},
                       {ex.data(), ex.size() * sizeof(ksim_label_expr)},
                       {tm.data(), tm.size() * sizeof(ksim_term)},
                       {nn.data(), 4 * nn.size()},
                       {bflag, sizeof(bflag)},
                       {&plan, sizeof(plan)},
                       {us.data(), us.size() * sizeof(ksim_topo_use)},
                       {ad.data(), ad.size() * sizeof(ksim_class_add)}};
  size_t total = 0;
  for (int q = 0; q < 8; q++) {
    b.off[q] = total;
    total += (std::max<size_t>(pc[q].bytes, 16) + 63) & ~(size_t)63;
  }
  b.bytes.assign(total, 0);                // zero padding: blobs of one pod compare equal (capacity reused)
  for (int q = 0; q < 8; q++)
    if (pc[q].bytes) std::memcpy(b.bytes.data() + b.off[q], pc[q].src, pc[q].bytes);
  b.n_nn = (int32_t)nn.size();
  b.n_exprs = (int32_t)ex.size();
  b.n_terms = (int32_t)tm.size();
  b.n_uses = (int32_t)us.size();
  b.n_adds = (int32_t)ad.size();
}

// The device pod set of a blob uploaded at d.
static DevPods blob_pods(const ksim_handle* h, const PodBlob& b, char* d) {
  DevPods P{};
  P.pods = (const ksim_pod*)(d + b.off[0]);
  P.exprs = (const ksim_label_expr*)(d + b.off[1]);
  P.terms = (const ksim_term*)(d + b.off[2]);
  P.nn = (const int32_t*)(d + b.off[3]);
  P.n_nn = b.n_nn;
  P.bflags = (const int32_t*)(d + b.off[4]);
  P.plans = (const PodPlan*)(d + b.off[5]);
  P.uses = (const ksim_topo_use*)(d + b.off[6]);
  P.adds = (const ksim_class_add*)(d + b.off[7]);
  P.n_pods = 1;
  P.n_exprs = b.n_exprs;
  P.n_terms = b.n_terms;
  // this pod's binds keep the loaded queue's persistent tables (its plan reads
  // none of them: no kPlanPtab on single uploads)
  P.ptab = h->dp.ptab;
  P.ptab_ent = h->dp.ptab_ent;
  P.ptab_cfirst = h->dp.ptab_cfirst;
  P.ptab_cidx = h->dp.ptab_cidx;
  P.n_uses = b.n_uses;
  P.n_adds = b.n_adds;
  return P;
}

// The blob into the pinned staging and, by one copy kernel, into the arena
// (valid until the arena's next upload).  The staging is reused once the last
// upload's copy has run (its event), not after the whole stream drains; a
// growing staging or arena drains the stream first.  begin_win: a
// framework-driven filter pass's start in the same launch.
// The next slot of the upload ring, free (its last copy has run) and at least
// `bytes` large.
static int ring_slot(ksim_handle* h, size_t bytes, ksim_handle::PinSlot** out) {
  ksim_handle::PinSlot& sl = h->ring[h->ring_next];
  h->ring_next = (h->ring_next + 1) % ksim_handle::kPinRing;
  if (sl.pending) HIPCHK(h, hipEventSynchronize(sl.ev));   // this slot's last reader (four uploads ago)
  sl.pending = false;
  if (const int rc = sl.buf.reserve(h, bytes, Idle::kCaller)) return rc;   // its reader has run, above
  *out = &sl;
  return KSIM_OK;
}

static int upload_blob(ksim_handle* h, const PodBlob& b, DevGrow& arena, DevPods& P,
                       WinState* begin_win = nullptr, bool record = false, bool synced = false) {
  const size_t total = b.bytes.size();
  if (h->pend_bind.on && arena.p && (const char*)h->pend_bind.P.pods >= (const char*)arena.p &&
      (const char*)h->pend_bind.P.pods < (const char*)arena.p + arena.cap) {
    // the queued Reserve reads this arena (every caller alternates arenas, so
    // this does not happen today): land it before the arena is grown or overwritten
    h->pend_reuse++;
    if (const int prc = flush_pend_bind(h)) return prc;
  }
  if (total > arena.cap) {
    HIPCHK(h, hipStreamSynchronize(h->stream));   // the arena is reallocated: nothing may read it
    for (auto& r : h->ring) r.pending = false;
  }
  ksim_handle::PinSlot* slp = nullptr;
  int rc;
  if ((rc = ring_slot(h, total, &slp))) return rc;
  ksim_handle::PinSlot& sl = *slp;
  if ((rc = arena.reserve(h, total, Idle::kCaller))) return rc;   // drained above when it grows
  std::memcpy(sl.buf.p, b.bytes.data(), total);
  Copies cp;
  cp.add(sl.buf.d, arena.p, total);
  if (begin_win) cp.begin(h->st, begin_win, 0, 1);
  if (record && h->pend_bind.on) {         // the last cycle's queued Reserve, ahead of this pass
    cp.bind(h->dc, h->pend_bind.P, h->pend_bind.node, h->pend_bind.sign);
    h->pend_bind.on = false;
  }
  if ((rc = cp.run(h))) return rc;
  if (!synced) {                           // synced: the caller drains the stream before returning
    if (!sl.ev) HIPCHK(h, hipEventCreateWithFlags(sl.ev.out(), hipEventDisableTiming));
    HIPCHK(h, hipEventRecord(sl.ev, h->stream));
    sl.pending = true;
  }
  P = blob_pods(h, b, (char*)arena.p);
  if (record || &arena == &h->pod1_arena) {   // what a Reserve of this pod binds from
    h->pod1_blob = b.bytes;
    h->pod1_base = (char*)arena.p;
  }
  return KSIM_OK;
}

// Upload one pod (re-based) as a device pod set of its own.
int ksim_host::upload_single(ksim_handle* h, const ksim_pod_set* ps, int32_t pod_index, DevPods& P, DevGrow& arena) {
  PodBlob b;
  build_pod_blob(h, ps, pod_index, b);
  return upload_blob(h, b, arena, P);
}

int ksim_host::upload_single(ksim_handle* h, const ksim_pod_set* ps, int32_t pod_index, DevPods& P) {
  return upload_single(h, ps, pod_index, P, h->pod1_arena);
}

int ksim_host::upload_many(ksim_handle* h, const ksim_pod_set* ps, const int32_t* idx, int32_t n, size_t extra,
                           std::vector<DevPods>& Ps, char** extra_host, char** extra_dev) {
  std::vector<PodBlob> blobs((size_t)n);
  std::vector<size_t> at((size_t)n);
  size_t total = 0;
  for (int32_t i = 0; i < n; i++) {
    build_pod_blob(h, ps, idx[i], blobs[i]);
    at[i] = total;
    total += (blobs[i].bytes.size() + 63) & ~(size_t)63;
  }
  int rc;
  if ((rc = h->many_arena.reserve(h, total + extra, Idle::kSync)) ||   // reallocated: nothing may read them
      (rc = h->many_stage.reserve(h, total + extra, Idle::kSync)))
    return rc;
  char* stage = (char*)h->many_stage.p;
  std::memset(stage, 0, total + extra);
  Ps.resize((size_t)n);
  char* d = (char*)h->many_arena.p;
  for (int32_t i = 0; i < n; i++) {
    std::memcpy(stage + at[i], blobs[i].bytes.data(), blobs[i].bytes.size());
    Ps[i] = blob_pods(h, blobs[i], d + at[i]);
  }
  h->many_stage_bytes = total + extra;
  *extra_host = stage + total;
  *extra_dev = d + total;
  return KSIM_OK;
}

int ksim_host::upload_many_commit(ksim_handle* h) {
  if (h->many_stage_bytes)
    HIPCHK(h, hipMemcpyAsync(h->many_arena.p, h->many_stage.p, h->many_stage_bytes, hipMemcpyHostToDevice, h->stream));
  return KSIM_OK;
}

// Copy one compat cycle's per-node outputs and scalars to the caller.
// The device marks a node whose Filter status was an error with kFailError
// next to the plugin index; the ABI reports the plugin index alone (the cycle
// status says the cycle failed).
static void strip_fail_errors(uint8_t* f, size_t n) {
  for (size_t i = 0; i < n; i++)
    if (fail_is_error(f[i])) f[i] &= (uint8_t)~kFailError;
}

static int copy_eval_out(ksim_handle* h, ksim_eval_out* out) {
  const size_t N = (size_t)h->dc.n;
  const int S = h->prof.n_score;
  if (out->fail_plugin) {
    HIPCHK(h, hcopy(h, out->fail_plugin, h->sc.fail, N, hipMemcpyDeviceToHost));
    strip_fail_errors(out->fail_plugin, N);
  }
  if (out->fail_detail) HIPCHK(h, hcopy(h, out->fail_detail, h->sc.detail, 4 * N, hipMemcpyDeviceToHost));
  if (out->scored) HIPCHK(h, hcopy(h, out->scored, h->eo.scored, N, hipMemcpyDeviceToHost));
  if (out->raw && S) HIPCHK(h, hcopy(h, out->raw, h->eo.raw, 8 * N * S, hipMemcpyDeviceToHost));
  if (out->norm && S) HIPCHK(h, hcopy(h, out->norm, h->eo.norm, 8 * N * S, hipMemcpyDeviceToHost));
  if (out->total) HIPCHK(h, hcopy(h, out->total, h->eo.total, 8 * N, hipMemcpyDeviceToHost));
  DevState st;
  HIPCHK(h, hcopy(h, &st, h->st, sizeof(st), hipMemcpyDeviceToHost));
  out->chosen = st.chosen;
  out->status = st.status;
  out->n_feasible = st.n_feasible;
  out->n_evaluated = st.n_evaluated;
  out->n_processed = st.n_processed;
  out->k_to_find = st.k_to_find;
  out->next_start = st.next_start_after;
  if (out->scored && out->n_feasible <= 1) std::memset(out->scored, 0, N);
  return KSIM_OK;
}

int ksim_eval_pod(ksim_handle* h, const ksim_pod_set* ps, int32_t pod_index, ksim_eval_out* out) {
  int rc = ensure_ready(h);
  if (rc) return rc;
  if (!ps || !out || pod_index < 0 || pod_index >= ps->n_pods || !ps->pods)
    return set_err(h, KSIM_E_INVALID, "bad pod set / index");
  if ((rc = validate_pod(h, ps, pod_index))) return rc;
  if (is_sharded(h) && profile_nb(h->prof))
    return set_err(h, KSIM_E_UNSUPPORTED, "NetworkBandwidth profiles run on unsharded handles");
  HIPCHK(h, hipSetDevice(h->device));
  h->ext_pending = false;
  DevPods P;
  if ((rc = upload_single(h, ps, pod_index, P))) return rc;
  if ((rc = set_run(h, 0, 1))) return rc;
  launch_cycle(make_args(h, P, nullptr), h->stream, true, ps->pods[pod_index].use_count > 0);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return copy_eval_out(h, out);
}

int ksim_eval_pod_filter(ksim_handle* h, const ksim_pod_set* ps, int32_t pod_index, ksim_eval_out* out) {
  int rc = ensure_ready(h);
  if (rc) return rc;
  if (!ps || !out || pod_index < 0 || pod_index >= ps->n_pods || !ps->pods)
    return set_err(h, KSIM_E_INVALID, "bad pod set / index");
  if (is_sharded(h)) return set_err(h, KSIM_E_UNSUPPORTED, "extender cycles run on unsharded handles");
  if ((rc = validate_pod(h, ps, pod_index))) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  if ((rc = upload_single(h, ps, pod_index, h->pod1))) return rc;
  if ((rc = set_run(h, 0, 1))) return rc;
  launch_cycle_filter(make_args(h, h->pod1, nullptr), h->stream, ps->pods[pod_index].use_count > 0);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipStreamSynchronize(h->stream));
  const size_t N = (size_t)h->dc.n;
  if (out->fail_plugin) {
    HIPCHK(h, hcopy(h, out->fail_plugin, h->sc.fail, N, hipMemcpyDeviceToHost));
    strip_fail_errors(out->fail_plugin, N);
  }
  if (out->fail_detail) HIPCHK(h, hcopy(h, out->fail_detail, h->sc.detail, 4 * N, hipMemcpyDeviceToHost));
  WinState w;
  DevState st;
  HIPCHK(h, hcopy(h, &w, h->sc.win, sizeof(w), hipMemcpyDeviceToHost));
  HIPCHK(h, hcopy(h, &st, h->st, sizeof(st), hipMemcpyDeviceToHost));
  const int32_t ns = w.nscan;                      // nodes scanned (PreFilterResult: its node count)
  const int32_t processed = w.cut < ns ? w.cut : ns;
  out->chosen = w.error ? KSIM_CHOSEN_ERROR : -1;
  out->status = w.error ? KSIM_STATUS_ERROR : 0;
  out->n_feasible = w.nf;
  out->n_evaluated = w.evaluated;
  out->n_processed = processed;
  out->k_to_find = w.k;
  out->next_start = ns > 0 ? (int32_t)(((int64_t)st.next_start + processed) % ns) : st.next_start;
  h->ext_pending = true;
  return KSIM_OK;
}

int ksim_eval_pod_finish(ksim_handle* h, const uint8_t* ext_fail, const int64_t* ext_score, ksim_eval_out* out) {
  int rc = ensure_ready(h);
  if (rc) return rc;
  if (!out) return set_err(h, KSIM_E_INVALID, "out is null");
  if (!h->ext_pending) return set_err(h, KSIM_E_INVALID, "ksim_eval_pod_finish without ksim_eval_pod_filter");
  h->ext_pending = false;
  HIPCHK(h, hipSetDevice(h->device));
  const size_t N = (size_t)h->dc.n;
  if (ext_fail)
    HIPCHK(h, hipMemcpyAsync(h->ext_fail, ext_fail, N, hipMemcpyHostToDevice, h->stream));
  else
    HIPCHK(h, hipMemsetAsync(h->ext_fail, 0, N, h->stream));
  if (ext_score)
    HIPCHK(h, hipMemcpyAsync(h->ext_score, ext_score, 8 * N, hipMemcpyHostToDevice, h->stream));
  else
    HIPCHK(h, hipMemsetAsync(h->ext_score, 0, 8 * N, h->stream));
  LaunchArgs a = make_args(h, h->pod1, nullptr);
  a.s.ext_fail = h->ext_fail;
  a.s.ext_score = h->ext_score;
  launch_cycle_finish(a, h->stream);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return copy_eval_out(h, out);
}

// ---- framework-driven compat mode (SURVEY §8(b) compat mode) -------------------
// The simulator runs upstream's framework with parallelism 16 and
// percentageOfNodesToScore 0 (simulator/scheduler/scheduler.go:149,153,231-241):
// the framework, not the engine, decides which nodes Filter runs on, the list
// PreScore / Score / NormalizeScore see and the node Reserve records
// (wrappedplugin.go:356-375, 491-516, 583-584).  These entry points answer the
// engine-backed plugins under those choices.
int ksim_fw_prefilter(ksim_handle* h, const ksim_pod_set* ps, int32_t pod_index, ksim_eval_out* out) {
  // a queued Reserve of the last cycle runs inside this pass's upload launch;
  // with Unreserves queued behind it (deferred_binds) it is launched first
  if (h && h->pend_bind.on && !h->deferred_binds.empty()) {
    const int prc = flush_pend_bind(h);
    if (prc) return prc;
  }
  int rc = ensure_ready(h, false, true);   // abandons any framework cycle in flight
  if (rc) return rc;
  if (!ps || !out || pod_index < 0 || pod_index >= ps->n_pods || !ps->pods)
    return set_err(h, KSIM_E_INVALID, "bad pod set / index");
  if (is_sharded(h)) return set_err(h, KSIM_E_UNSUPPORTED, "framework-driven cycles run on unsharded handles");
  if ((rc = validate_pod(h, ps, pod_index))) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  h->ext_pending = false;
  h->fw_list.clear();                // a new cycle: no normalization answered from the last one
  h->fw_raw.clear();
  const ksim_pod& p = ps->pods[pod_index];
  const size_t N = (size_t)h->dc.n;
  const int S = h->prof.n_score;
  // Score on the host (ksim_fw_score) unless a PreScore reads the framework's
  // list: PodTopologySpread's ScheduleAnyway constraints (IgnoredNodes, pair
  // counts over the list); NetworkBandwidth's Score may fail the cycle
  bool host = S > 0 && !profile_nb(h->prof) && !(p.flags & KSIM_POD_NODE_NAMES_UNKNOWN);
  for (int32_t u = 0; host && u < p.use_count; u++)
    if (ps->uses[p.use_first + u].kind == KSIM_USE_PTS_SOFT) host = false;
  h->fw_host = host;
  // a pod without topology uses: the filter kernel writes its answers straight
  // to the pinned staging (fwh), no copy launch; with uses, the topology flags
  // are the PreFilter pass's, copied after it
  const bool mirror = p.use_count == 0;
  // fwh: [head 64][fail N][detail 4N][raw S x N][part N], 64-byte aligned pieces
  const size_t o_fail = 64, o_det = o_fail + ((N + 63) & ~(size_t)63),
               o_raw = o_det + ((4 * N + 63) & ~(size_t)63), o_part = o_raw + ((8 * (size_t)S * N + 63) & ~(size_t)63),
               need = o_part + 8 * N;
  if ((rc = h->fwh.reserve(h, need, Idle::kSync))) return rc;
  char* fo = (char*)h->fwh.p;
  char* fd = (char*)h->fwh.d;
  // the pod, and the run header / window state / topology flags reset, in one
  // launch (upload_blob's begin job)
  build_pod_blob(h, ps, pod_index, h->fw_blob);
  h->fw_flip ^= 1;
  if ((rc = upload_blob(h, h->fw_blob, h->fw_arena[h->fw_flip], h->pod1, h->sc.win, true, true))) return rc;
  LaunchArgs a = make_args(h, h->pod1, nullptr);
  if (mirror) {
    a.s.m_head = (int32_t*)fd;
    a.s.m_fail = (uint8_t*)(fd + o_fail);
    a.s.m_detail = out->fail_detail ? (uint32_t*)(fd + o_det) : nullptr;
    a.s.m_raw = host ? (int32_t*)(fd + o_raw) : nullptr;
    reinterpret_cast<int32_t*>(fo)[1] = 0;        // the kernel's too-wide flag
  }
  launch_fw_filter(a, h->stream, p.use_count > 0);
  HIPCHK(h, hipGetLastError());
  h->fw_dom_dirty = p.use_count > 0;
  h->fw_topo = p.use_count > 0;
  h->fw_fail.resize(N);
  if (!mirror) {
    // the results into the same staging, one copy launch: next_start, the
    // topology flags, the filter codes, the details (and the raw scores)
    Copies cp;
    cp.add(&h->st->next_start, fd, sizeof(int32_t));
    cp.add(&h->st->topo_flags, fd + 4, sizeof(uint32_t));
    cp.add(h->sc.fail, fd + o_fail, N);
    if (out->fail_detail) cp.add(h->sc.detail, fd + o_det, 4 * N);
    if (host) {
      cp.add(h->sc.raw, fd + o_raw, 8 * (size_t)S * N);
      cp.add(h->sc.part, fd + o_part, 8 * N);
    }
    if ((rc = cp.run(h))) return rc;
  }
  HIPCHK(h, hipStreamSynchronize(h->stream));
  std::memcpy(h->fw_fail.data(), fo + o_fail, N);
  if (out->fail_detail) std::memcpy(out->fail_detail, fo + o_det, 4 * N);
  int32_t ns = h->dc.n;
  if (p.flags & KSIM_POD_NODE_NAMES) ns = (p.flags & KSIM_POD_NODE_NAMES_UNKNOWN) ? 0 : p.nn_count;
  int32_t nf = 0;
  for (size_t i = 0; i < N; i++) nf += h->fw_fail[i] == KSIM_PASSED;
  if (out->fail_plugin) {
    std::memcpy(out->fail_plugin, h->fw_fail.data(), N);
    strip_fail_errors(out->fail_plugin, N);
  }
  int32_t next = 0;
  std::memcpy(&next, fo, sizeof(next));
  h->fw_tflags = 0;
  if (!mirror) std::memcpy(&h->fw_tflags, fo + 4, sizeof(uint32_t));
  h->fw_oraw = o_raw;
  h->fw_opart = o_part;
  h->fw_raw32 = mirror;
  if (mirror && host && reinterpret_cast<const int32_t*>(fo)[1] != 0)
    h->fw_host = false;                  // a raw score past int32: ksim_fw_score on the device
  const bool unknown = (p.flags & KSIM_POD_NODE_NAMES_UNKNOWN) != 0;
  out->chosen = unknown ? KSIM_CHOSEN_ERROR : -1;
  out->status = unknown ? KSIM_STATUS_ERROR : 0;
  out->n_feasible = nf;
  out->n_evaluated = ns;
  out->n_processed = 0;
  out->k_to_find = num_feasible_nodes_to_find(h->prof.percentage_of_nodes_to_score, ns);
  out->next_start = next;
  h->fw_ns = ns;
  h->fw_pending = !unknown;
  return KSIM_OK;
}

// The cycle's filter pass again, on the current dynamic state: the PreFilter
// domain sums start from zero, the topology flags too (ksim_fw_prefilter).
static int fw_filter_pass(ksim_handle* h) {
  if (h->fw_topo && h->sc.dom)
    HIPCHK(h, hipMemsetAsync(h->sc.dom, 0, 8 * (size_t)KSIM_MAX_USES * h->dc.vmax, h->stream));
  launch_fw_begin(h->st, h->sc.win, 0, 1, h->stream);
  launch_fw_filter(make_args(h, h->pod1, nullptr), h->stream, h->fw_topo);
  HIPCHK(h, hipGetLastError());
  return KSIM_OK;
}

// RunFilterPluginsWithNominatedPods' first pass: for each listed node, the
// cycle's pod against that node with its nominated pods added (addNominatedPods:
// NodeInfo.AddPodInfo and the PreFilterExtensions' AddPod of PodTopologySpread
// and InterPodAffinity, which for +1 updates equal a PreFilter over the state
// with the pods bound there).  Each node's pods are assumed, the filter pass
// re-run, the node's verdict read, the pods forgotten; a last pass restores the
// cycle's own PreFilter state for ksim_fw_score.
int ksim_fw_filter_nominated(ksim_handle* h, const ksim_pod_set* nps, int32_t n_nodes, const int32_t* nodes,
                             const int32_t* first, const int32_t* count, uint8_t* fail_plugin,
                             uint32_t* fail_detail) {
  int rc = ensure_ready(h, true);
  if (rc) return rc;
  if (!h->fw_pending) return set_err(h, KSIM_E_INVALID, "ksim_fw_filter_nominated without ksim_fw_prefilter");
  if (n_nodes < 0 || (n_nodes > 0 && (!nodes || !first || !count || !nps || !nps->pods || !fail_plugin)))
    return set_err(h, KSIM_E_INVALID, "bad nominated-node groups");
  for (int32_t k = 0; k < n_nodes; k++) {
    if (nodes[k] < 0 || nodes[k] >= h->dc.n) return set_err(h, KSIM_E_INVALID, "nominated node out of range");
    if (count[k] < 0 || first[k] < 0 || first[k] + count[k] > nps->n_pods)
      return set_err(h, KSIM_E_INVALID, "nominated pod range out of the pod set");
    for (int32_t j = first[k]; j < first[k] + count[k]; j++)
      if ((rc = validate_pod(h, nps, j))) return rc;
  }
  if (n_nodes == 0) return KSIM_OK;
  HIPCHK(h, hipSetDevice(h->device));
  auto bind_all = [&](int32_t k, int sign) -> int {
    for (int32_t j = first[k]; j < first[k] + count[k]; j++) {
      DevPods P;
      int r;
      if ((r = upload_single(h, nps, j, P, h->nom_arena))) return r;
      launch_assume(h->dc, P, 0, nodes[k], sign, h->stream);
      HIPCHK(h, hipGetLastError());
    }
    return KSIM_OK;
  };
  for (int32_t k = 0; k < n_nodes; k++) {
    if ((rc = bind_all(k, 1))) return rc;
    if ((rc = fw_filter_pass(h))) return rc;
    uint8_t f = 0;
    uint32_t d = 0;
    HIPCHK(h, hcopy(h, &f, h->sc.fail + nodes[k], 1, hipMemcpyDeviceToHost));
    HIPCHK(h, hcopy(h, &d, h->sc.detail + nodes[k], 4, hipMemcpyDeviceToHost));
    if (fail_is_error(f)) f &= (uint8_t)~kFailError;
    fail_plugin[k] = f;
    if (fail_detail) fail_detail[k] = d;
    if ((rc = bind_all(k, -1))) return rc;
  }
  if ((rc = fw_filter_pass(h))) return rc;                 // the cycle's own PreFilter state again
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return KSIM_OK;
}

// NormalizeScore of one value on the host (ksim_device.h normalize_value, the
// same integer and float64 expressions; -ffp-contract=off holds for this file)
static int64_t host_normalize(int32_t kind, int64_t v, int64_t gmax, int64_t gmin, bool ipa_nonempty) {
  switch (kind) {
    case kNormDefault: {
      const int64_t m = gmax > 0 ? gmax : 0;
      return m == 0 ? v : (int64_t)((uint64_t)kMaxNodeScore * (uint64_t)v) / m;
    }
    case kNormDefaultReverse: {
      const int64_t m = gmax > 0 ? gmax : 0;
      return m == 0 ? (int64_t)kMaxNodeScore : (int64_t)kMaxNodeScore - (int64_t)((uint64_t)kMaxNodeScore * (uint64_t)v) / m;
    }
    case kNormPTS: {
      const int64_t mx = gmax > 0 ? gmax : 0;
      return mx == 0 ? (int64_t)kMaxNodeScore : (int64_t)((uint64_t)kMaxNodeScore * (uint64_t)(mx + gmin - v)) / mx;
    }
    case kNormIPA:
    case kNormMinMax: {
      if (kind == kNormIPA && !ipa_nonempty) return v;
      const int64_t diff = gmax - gmin;
      double f = 0;
      if (diff > 0) f = (double)kMaxNodeScore * ((double)(v - gmin) / (double)diff);
      return (int64_t)f;
    }
    default:
      return v;
  }
}

// ksim_fw_score answered on the host (fw_host): PreScore / Score were the
// filter pass's (no list-dependent PreScore), NormalizeScore, the weights and
// the totals over the framework's list, as k_window / k_extrema / k_select
// compute them (k_select: one listed node is not scored).
static int fw_score_host(ksim_handle* h, const int32_t* nodes, int32_t n, ksim_eval_out* out) {
  const size_t N = (size_t)h->dc.n;
  const int S = h->prof.n_score;
  std::vector<uint8_t>& seen = h->fw_seen;
  if (seen.size() != N) seen.assign(N, 0);
  for (int32_t j = 0; j < n; j++) {
    const int32_t x = nodes[j];
    if (x < 0 || (size_t)x >= N || h->fw_fail[x] != KSIM_PASSED || seen[x]) {
      for (int32_t q = 0; q < j; q++) seen[nodes[q]] = 0;
      return set_err(h, KSIM_E_INVALID, "node list: not a feasible node of the filter pass, or repeated");
    }
    seen[x] = 1;
  }
  for (int32_t j = 0; j < n; j++) seen[nodes[j]] = 0;
  // the filter pass's answers: node-major int32 rows [n][S + 1] (the kernel's
  // own copy), or slot-major int64 [S][n] and [n] (a copy launch)
  const char* rawb = (const char*)h->fwh.p + h->fw_oraw;
  const char* partb = (const char*)h->fwh.p + h->fw_opart;
  const bool w32 = h->fw_raw32;
  const size_t W = (size_t)S + 1;
  auto raw_at = [&](int k, size_t node) -> int64_t {
    return w32 ? (int64_t)reinterpret_cast<const int32_t*>(rawb)[node * W + (size_t)k]
               : reinterpret_cast<const int64_t*>(rawb)[(size_t)k * N + node];
  };
  auto part_at = [&](size_t node) -> int64_t {
    return w32 ? (int64_t)reinterpret_cast<const int32_t*>(rawb)[node * W + (size_t)S]
               : reinterpret_cast<const int64_t*>(partb)[node];
  };
  const bool scored = n > 1;
  const bool ipa_nonempty = (h->fw_tflags & kTopoScoreNonEmpty) != 0;
  h->fw_list.assign(nodes, nodes + n);
  h->fw_raw.assign((size_t)S * n, 0);
  h->fw_norm.assign((size_t)S * n, 0);
  std::vector<int64_t>& tot = h->fw_tot;
  tot.assign(n, 0);
  if (scored) {
    if (w32) {                             // one row (a cache line) per listed node
      const int32_t* rows = reinterpret_cast<const int32_t*>(rawb);
      int64_t* fr = h->fw_raw.data();
      for (int32_t j = 0; j < n; j++) {
        const int32_t* row = rows + (size_t)nodes[j] * W;
        for (int k = 0; k < S; k++) fr[(size_t)k * n + j] = row[k];
        tot[j] = row[S];
      }
    } else {
      for (int32_t j = 0; j < n; j++) tot[j] = part_at((size_t)nodes[j]);
      for (int k = 0; k < S; k++)
        for (int32_t j = 0; j < n; j++) h->fw_raw[(size_t)k * n + j] = raw_at(k, (size_t)nodes[j]);
    }
    for (int k = 0; k < S; k++) {
      int64_t* r = h->fw_raw.data() + (size_t)k * n;
      int64_t* nv = h->fw_norm.data() + (size_t)k * n;
      const int32_t kind = norm_kind(h->prof.score[k]);
      if (kind == kNormNone) {
        std::memcpy(nv, r, 8 * (size_t)n);
        continue;
      }
      int64_t gmax = INT64_MIN, gmin = INT64_MAX;
      for (int32_t j = 0; j < n; j++) {
        gmax = std::max(gmax, r[j]);
        gmin = std::min(gmin, r[j]);
      }
      const int64_t w = h->prof.score_weight[k] == 0 ? 1 : h->prof.score_weight[k];
      // a list's raw scores take few distinct values: each value's normalized
      // score once (a 64-entry direct-mapped memo), not a division per node
      int64_t mk[64], mv[64];
      bool mset[64] = {};
      for (int32_t j = 0; j < n; j++) {
        const int64_t v = r[j];
        const uint32_t e = (uint32_t)((uint64_t)v * 0x9E3779B97F4A7C15ull >> 58);
        if (!mset[e] || mk[e] != v) {
          mset[e] = true;
          mk[e] = v;
          mv[e] = host_normalize(kind, v, gmax, gmin, ipa_nonempty);
        }
        nv[j] = mv[e];
        tot[j] += mv[e] * w;
      }
    }
  }
  if (out->scored)
    for (int32_t j = 0; j < n; j++) out->scored[nodes[j]] = scored ? 1 : 0;
  for (int k = 0; k < S; k++) {
    if (out->raw) {
      int64_t* r = out->raw + (size_t)k * N;
      for (int32_t j = 0; j < n; j++) r[nodes[j]] = h->fw_raw[(size_t)k * n + j];
    }
    if (out->norm) {
      int64_t* r = out->norm + (size_t)k * N;
      for (int32_t j = 0; j < n; j++) r[nodes[j]] = h->fw_norm[(size_t)k * n + j];
    }
  }
  if (out->total)
    for (int32_t j = 0; j < n; j++) out->total[nodes[j]] = tot[j];
  if (out->fail_plugin) {                  // the filter pass, unchanged
    std::memcpy(out->fail_plugin, h->fw_fail.data(), N);
    strip_fail_errors(out->fail_plugin, N);
  }
  out->n_feasible = n;
  out->n_evaluated = h->fw_ns;
  out->n_processed = 0;
  out->k_to_find = num_feasible_nodes_to_find(h->prof.percentage_of_nodes_to_score, h->fw_ns);
  out->chosen = -1;
  out->status = 0;
  h->fw_pending = false;                   // the domain sums stay for fw_abandon (no k_select ran)
  h->fw_scored = true;
  return KSIM_OK;
}

int ksim_fw_score(ksim_handle* h, const int32_t* nodes, int32_t n, ksim_eval_out* out) {
  int rc = ensure_ready(h, true);
  if (rc) return rc;
  if (!out || n < 0 || (n > 0 && !nodes)) return set_err(h, KSIM_E_INVALID, "bad node list");
  if (!h->fw_pending) return set_err(h, KSIM_E_INVALID, "ksim_fw_score without ksim_fw_prefilter");
  h->fw_counts[h->fw_host ? 0 : 1]++;
  if (h->fw_host) return fw_score_host(h, nodes, n, out);
  const size_t N = (size_t)h->dc.n;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));    // the upload staging is free again
  const size_t o_list = (64 + N + 63) & ~(size_t)63;
  if ((rc = h->pin.reserve(h, o_list + 4 * (size_t)n, Idle::kCaller))) return rc;   // idle: drained above
  // the list: feasible nodes of the filter pass, each once (the mask in staging)
  uint8_t* out_of_list = (uint8_t*)h->pin.p + 64;
  std::memset(out_of_list, 1, N);
  for (int32_t j = 0; j < n; j++) {
    const int32_t x = nodes[j];
    if (x < 0 || (size_t)x >= N || h->fw_fail[x] != KSIM_PASSED || !out_of_list[x])
      return set_err(h, KSIM_E_INVALID, "node list: not a feasible node of the filter pass, or repeated");
    out_of_list[x] = 0;
  }
  std::memcpy((char*)h->pin.p + o_list, nodes, 4 * (size_t)n);
  // the window of the filter pass covers the whole scan set (k_window's
  // extender branch keeps it and drops the unlisted nodes)
  std::memcpy(h->pin.p, &h->fw_ns, sizeof(int32_t));
  {
    Copies cp;
    cp.add((char*)h->pin.d + 64, h->ext_fail, N);
    cp.add(h->pin.d, &h->sc.win->cut, sizeof(int32_t));
    cp.add((char*)h->pin.d + o_list, h->fw_nodes, 4 * (size_t)n);
    if ((rc = cp.run(h))) return rc;
  }
  LaunchArgs a = make_args(h, h->pod1, nullptr);
  a.s.ext_fail = h->ext_fail;
  a.s.ext_score = nullptr;
  launch_fw_score(a, h->stream);
  const int S = h->prof.n_score;
  // the listed nodes' answers and the window state gathered straight into
  // the pinned staging, one synchronization; the caller's entries of
  // unlisted nodes are left as they are (ksim_engine.h)
  const size_t o_comp = (sizeof(WinState) + 63) & ~(size_t)63, nb = (16 * (size_t)S + 9) * n;
  if ((rc = h->pout.reserve(h, o_comp + nb, Idle::kSync))) return rc;
  char* po = (char*)h->pout.p;
  launch_fw_gather(h->eo, h->fw_nodes, n, (int32_t)N, S, (int64_t*)((char*)h->pout.d + o_comp), h->sc.win,
                   h->pout.d, h->stream);
  HIPCHK(h, hipGetLastError());
  h->fw_pending = false;
  h->fw_dom_dirty = false;                 // k_select re-zeroed the domain sums
  h->fw_scored = true;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  const int64_t* craw = (const int64_t*)(po + o_comp);
  const int64_t* cnorm = craw + (size_t)S * n;
  const int64_t* ctot = cnorm + (size_t)S * n;
  const uint8_t* csc = (const uint8_t*)(ctot + n);
  if (out->scored)
    for (int32_t j = 0; j < n; j++) out->scored[nodes[j]] = csc[j];
  for (int k = 0; k < S; k++) {
    if (out->raw) {
      int64_t* r = out->raw + (size_t)k * N;
      for (int32_t j = 0; j < n; j++) r[nodes[j]] = craw[(size_t)k * n + j];
    }
    if (out->norm) {
      int64_t* r = out->norm + (size_t)k * N;
      for (int32_t j = 0; j < n; j++) r[nodes[j]] = cnorm[(size_t)k * n + j];
    }
  }
  if (out->total)
    for (int32_t j = 0; j < n; j++) out->total[nodes[j]] = ctot[j];
  // kept for ksim_fw_normalize over the same list
  h->fw_list.assign(nodes, nodes + n);
  h->fw_raw.assign(craw, craw + (size_t)S * n);
  h->fw_norm.assign(cnorm, cnorm + (size_t)S * n);
  WinState w;
  std::memcpy(&w, po, sizeof(w));
  if (out->fail_plugin) {                  // the filter pass, unchanged
    std::memcpy(out->fail_plugin, h->fw_fail.data(), N);
    strip_fail_errors(out->fail_plugin, N);
  }
  out->n_feasible = w.nf;
  out->n_evaluated = h->fw_ns;
  out->n_processed = 0;
  out->k_to_find = num_feasible_nodes_to_find(h->prof.percentage_of_nodes_to_score, h->fw_ns);
  out->chosen = w.error ? KSIM_CHOSEN_ERROR : -1;
  out->status = w.error ? KSIM_STATUS_ERROR : 0;
  if (out->scored && w.nf <= 1)
    for (int32_t j = 0; j < n; j++) out->scored[nodes[j]] = 0;
  return KSIM_OK;
}

int ksim_fw_normalize(ksim_handle* h, int32_t score_slot, const int32_t* nodes, const int64_t* scores, int32_t n,
                      int64_t* out) {
  int rc = ensure_ready(h, true);
  if (rc) return rc;
  if (!h->fw_scored) return set_err(h, KSIM_E_INVALID, "ksim_fw_normalize without ksim_fw_score");
  if (score_slot < 0 || score_slot >= h->prof.n_score) return set_err(h, KSIM_E_INVALID, "bad score slot");
  const size_t N = (size_t)h->dc.n;
  if (n < 0 || (size_t)n > N || (n > 0 && (!nodes || !scores || !out)))
    return set_err(h, KSIM_E_INVALID, "bad score list");
  for (int32_t j = 0; j < n; j++)
    if (nodes[j] < 0 || (size_t)nodes[j] >= N) return set_err(h, KSIM_E_INVALID, "bad node in score list");
  if (n == 0) return KSIM_OK;
  // the framework's NormalizeScore hands over exactly ksim_fw_score's list
  // and the raw scores it returned: that normalization is already computed
  if ((size_t)n == h->fw_list.size() && h->fw_raw.size() == (size_t)h->prof.n_score * n) {
    const int64_t* raw = h->fw_raw.data() + (size_t)score_slot * n;
    bool same = std::equal(nodes, nodes + n, h->fw_list.begin());
    for (int32_t j = 0; same && j < n; j++) same = scores[j] == raw[j];
    if (same) {
      h->fw_counts[2]++;
      std::memcpy(out, h->fw_norm.data() + (size_t)score_slot * n, 8 * (size_t)n);
      return KSIM_OK;
    }
  }
  h->fw_counts[3]++;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));    // the staging is free again
  const size_t o_vals = (4 * (size_t)n + 63) & ~(size_t)63;
  if ((rc = h->pin.reserve(h, o_vals + 8 * (size_t)n, Idle::kCaller)) ||   // idle: drained above
      (rc = h->pout.reserve(h, 8 * (size_t)n, Idle::kSync)))
    return rc;
  std::memcpy(h->pin.p, nodes, 4 * (size_t)n);
  std::memcpy((char*)h->pin.p + o_vals, scores, 8 * (size_t)n);
  {
    Copies cp;
    cp.add(h->pin.d, h->fw_nodes, 4 * (size_t)n);
    cp.add((char*)h->pin.d + o_vals, h->fw_vals, 8 * (size_t)n);
    if ((rc = cp.run(h))) return rc;
  }
  launch_fw_normalize(make_args(h, h->pod1, nullptr), score_slot, h->fw_nodes, h->fw_vals, n, h->fw_out, h->stream);
  HIPCHK(h, hipGetLastError());
  {
    Copies cp;
    cp.add(h->fw_out, h->pout.d, 8 * (size_t)n);
    if ((rc = cp.run(h))) return rc;
  }
  HIPCHK(h, hipStreamSynchronize(h->stream));
  std::memcpy(out, h->pout.p, 8 * (size_t)n);
  return KSIM_OK;
}

// Reserve / Unreserve (wrappedplugin.go:583-584, 617), uploaded through their
// own arena (never the cycle's pod).  Unreserve never abandons a framework
// cycle in flight: between that cycle's PreFilter and Score it is queued and
// applied once the cycle has scored (ensure_ready), as upstream's cycle keeps
// the snapshot it started from while the cache takes the binding goroutine's
// ForgetPod.  Reserve is the end of a cycle (after Score, or with one
// feasible node, which the framework does not score): it closes the cycle,
// applies what was queued, then assumes.
static int apply_bind(ksim_handle* h, const ksim_pod_set* ps, int32_t pod_index, int32_t node, int sign) {
  DevPods P;
  int rc;
  if ((rc = flush_pend_bind(h))) return rc;
  PodBlob b;
  build_pod_blob(h, ps, pod_index, b);
  if (h->pod1_base && b.bytes == h->pod1_blob) {
    // the pod the last filter pass uploaded (the framework's Reserve of the
    // cycle's pod): bind from its arena copy, queued (pend_bind) until the
    // next call: the next framework-driven pass runs it inside its upload
    // launch (into the other arena), any other call launches it first
    h->pend_bind.P = blob_pods(h, b, h->pod1_base);
    h->pend_bind.node = node;
    h->pend_bind.sign = sign;
    h->pend_bind.on = true;
    return KSIM_OK;
  }
  // another pod's Reserve / Unreserve (an informer's pod delta, a forget): the
  // bind reads the pod straight from a pinned ring slot (mapped host memory):
  // one launch, no arena copy
  ksim_handle::PinSlot* sl = nullptr;
  if ((rc = ring_slot(h, b.bytes.size(), &sl))) return rc;
  std::memcpy(sl->buf.p, b.bytes.data(), b.bytes.size());
  P = blob_pods(h, b, (char*)sl->buf.d);
  launch_assume(h->dc, P, 0, node, sign, h->stream);
  HIPCHK(h, hipGetLastError());
  if (!sl->ev) HIPCHK(h, hipEventCreateWithFlags(sl->ev.out(), hipEventDisableTiming));
  HIPCHK(h, hipEventRecord(sl->ev, h->stream));
  sl->pending = true;
  // no synchronization: every later call is ordered after it on the stream
  return KSIM_OK;
}

// the queued Unreserves, when no framework cycle sits between PreFilter and
// Score (the state getters read the cache's view)
int ksim_host::flush_idle(ksim_handle* h) {
  int rc = flush_pend_bind(h);
  if (rc) return rc;
  return (!h->fw_pending && !h->deferred_binds.empty()) ? flush_deferred_binds(h) : KSIM_OK;
}

static int flush_deferred_binds(ksim_handle* h) {
  std::vector<ksim_handle::DeferredBind> q;
  q.swap(h->deferred_binds);
  HIPCHK(h, hipSetDevice(h->device));
  for (auto& d : q) {
    ksim_pod_set v{};
    v.n_pods = 1;
    v.pods = &d.pod;
    v.n_exprs = (int32_t)d.ex.size();
    v.exprs = d.ex.data();
    v.n_terms = (int32_t)d.tm.size();
    v.terms = d.tm.data();
    v.n_uses = (int32_t)d.us.size();
    v.uses = d.us.data();
    v.n_adds = (int32_t)d.ad.size();
    v.adds = d.ad.data();
    v.n_nn = (int32_t)d.nn.size();
    v.nn = d.nn.data();
    const int rc = apply_bind(h, &v, 0, d.node, d.sign);
    if (rc) return rc;
  }
  return KSIM_OK;
}

static int assume_common(ksim_handle* h, const ksim_pod_set* ps, int32_t pod_index, int32_t node, int sign) {
  int rc = ensure_ready(h, sign < 0);
  if (rc) return rc;
  if (!ps || !ps->pods || pod_index < 0 || pod_index >= ps->n_pods || node < 0 || node >= h->dc.n)
    return set_err(h, KSIM_E_INVALID, "bad pod / node");
  if ((rc = validate_pod(h, ps, pod_index))) return rc;
  if (h->fw_pending) {                     // Unreserve, a cycle between PreFilter and Score: queued
    ksim_handle::DeferredBind d;
    single_pod_set(ps, pod_index, d.pod, d.ex, d.tm, d.us, d.ad, d.nn);
    d.node = node;
    d.sign = sign;
    h->deferred_binds.push_back(std::move(d));
    return KSIM_OK;
  }
  HIPCHK(h, hipSetDevice(h->device));
  return apply_bind(h, ps, pod_index, node, sign);
}

int ksim_assume(ksim_handle* h, const ksim_pod_set* ps, int32_t pod_index, int32_t node) {
  return assume_common(h, ps, pod_index, node, 1);
}

int ksim_forget(ksim_handle* h, const ksim_pod_set* ps, int32_t pod_index, int32_t node) {
  return assume_common(h, ps, pod_index, node, -1);
}

// Persistent domain tables of a queue: which pods read every
// domain sum from a table kept by the binds, and the tables they need.
struct PtabRegistry {
  std::vector<int4> ent;                 // {class, column, kind, first entry}
  std::vector<int32_t> cfirst, cidx;     // CSR by class
  int64_t len = 0;                       // int64 entries
  std::vector<uint8_t> pod;              // per pod: kPlanPtab
  std::vector<uint32_t> mask;            // per pod: UseMasks.ptab
  std::vector<int4> padd;                // per pod: the table updates of its adds
  std::vector<int32_t> padd_first, padd_count;
};

// uses: the queue's device use copies (kUseUniqueCol marked); their _pad
// becomes the first entry of the use's table.  A pod qualifies when each of
// its domain sums is independent of the pod beyond (class, column): PTS hard
// constraints on keys every node carries with nodeInclusionPolicies that
// filter nothing here, InterPodAffinity terms; value-keyed ScheduleAnyway
// constraints keep k_topo_prefilter (k_extrema reads their sums).  Shard
// handles exchange per-cycle sums and build no tables.
static void build_ptab(const ksim_handle* h, const ksim_pod_set* ps, std::vector<ksim_topo_use>& uses,
                       PtabRegistry& R) {
  R = PtabRegistry{};
  R.pod.assign((size_t)ps->n_pods, 0);
  R.mask.assign((size_t)ps->n_pods, 0);
  // replicas (RCCL ones included) hold every node: their tables are whole
  if ((is_sharded(h) && !h->replicated) || ab(kAbPtab)) return;   // A/B form: per-cycle PreFilter sums
  std::map<std::tuple<int32_t, int32_t, int32_t>, int32_t> index;
  for (int32_t i = 0; i < ps->n_pods; i++) {
    const ksim_pod& p = ps->pods[i];
    if (p.use_count <= 0) continue;
    ksim_topo_use* U = uses.data() + p.use_first;
    const UseMasks m = use_masks(h->prof, U, p.use_count);
    const bool pod_aff = p.sel_count > 0 || (p.flags & KSIM_POD_HAS_REQUIRED_AFFINITY);
    int32_t kind[KSIM_MAX_USES];
    bool ok = true;
    for (int k = 0; k < p.use_count && ok; k++) {
      const ksim_topo_use& u = U[k];
      const uint32_t b = 1u << k;
      kind[k] = -1;
      if (u.col == KSIM_COL_NONE) continue;
      if (use_node_count(u)) {                   // the node's own count; a total for the emptiness test
        if ((m.aff | m.score) & b && u.cls >= 0) kind[k] = kPtabTotal;
        continue;
      }
      if (u.kind == KSIM_USE_PTS_SOFT) {
        ok = false;
      } else if (u.kind == KSIM_USE_PTS_HARD) {
        ok = h->col_total[u.col] && h->col_nvals[u.col] <= kFuseMinValues &&
             !((u.flags & KSIM_USEF_HONOR_AFFINITY) && pod_aff) &&
             !((u.flags & KSIM_USEF_HONOR_TAINTS) && !h->hard_taints.empty());
        kind[k] = kPtabMark;
      } else {
        ok = !((m.aff | m.score) & b) || h->col_nvals[u.col] <= kFuseMinValues;   // emptiness scans
        kind[k] = kPtabPlain;
      }
    }
    if (!ok) continue;
    for (int k = 0; k < p.use_count; k++) {
      if (kind[k] < 0) continue;
      ksim_topo_use& u = U[k];
      const auto key = std::make_tuple(u.cls, (int32_t)u.col, kind[k]);
      auto it = index.find(key);
      if (it == index.end()) {
        it = index.emplace(key, (int32_t)R.ent.size()).first;
        R.ent.push_back(make_int4(u.cls, (int32_t)u.col, kind[k], (int32_t)R.len));
        R.len += kind[k] == kPtabTotal ? 1 : h->col_nvals[u.col];
      }
      u._pad = R.ent[(size_t)it->second].w;
      if (kind[k] != kPtabTotal) R.mask[i] |= 1u << k;
    }
    R.pod[i] = 1;
  }
  R.padd_first.assign((size_t)ps->n_pods, 0);
  R.padd_count.assign((size_t)ps->n_pods, 0);
  if (R.ent.empty()) return;
  const int32_t C = h->dc.n_classes;
  R.cfirst.assign((size_t)C + 1, 0);
  for (const int4& e : R.ent)
    if (e.x >= 0) R.cfirst[(size_t)e.x + 1]++;
  for (int32_t c = 0; c < C; c++) R.cfirst[(size_t)c + 1] += R.cfirst[(size_t)c];
  R.cidx.assign((size_t)R.cfirst[(size_t)C], 0);
  std::vector<int32_t> fill(R.cfirst.begin(), R.cfirst.end() - 1);
  for (size_t e = 0; e < R.ent.size(); e++)
    if (R.ent[e].x >= 0) R.cidx[(size_t)fill[(size_t)R.ent[e].x]++] = (int32_t)e;
  for (int32_t i = 0; i < ps->n_pods; i++) {
    const ksim_pod& p = ps->pods[i];
    R.padd_first[(size_t)i] = (int32_t)R.padd.size();
    for (int32_t a = 0; a < p.add_count; a++) {
      const ksim_class_add& ad = ps->adds[p.add_first + a];
      for (int32_t e = R.cfirst[(size_t)ad.cls]; e < R.cfirst[(size_t)ad.cls + 1]; e++) {
        const int4& t = R.ent[(size_t)R.cidx[(size_t)e]];
        R.padd.push_back(make_int4(t.w, t.y, t.z, ad.count));
      }
    }
    R.padd_count[(size_t)i] = (int32_t)R.padd.size() - R.padd_first[(size_t)i];
  }
}

// A use of a topology batch pod that may read a class an earlier pod of its
// run adds (ksim_tbatch.hip k_tb_chain_pairs): a node-local one (the guessed
// node's own count, re-keyed there).  A domain-keyed use ends the run: pod
// k's bind moves a whole domain for pod j.  Re-checking DoNotSchedule domain
// verdicts per batch was built and measured on config 3 (profiles/r04/tbcap):
// once an app's zones are level, nearly every bind of the app flips a zone's
// verdict, so the crossing pods were cut (pinv) after their evaluation was
// paid for (61.6 ms per step without crossing, 68.6-81.4 ms with).
static bool tbatch_conflict_ok(const ksim_topo_use& u) {
  return use_node_count(u) && u.kind != KSIM_USE_PTS_HARD && u.kind != KSIM_USE_NODE_PORT &&
         u.kind != KSIM_USE_IMAGE;
}

// The zone-variant use of a topology batch pod (ksim_device.h TbVar), or -1:
// its first DoNotSchedule spread use, read from a persistent table, keyed by a
// column of at most kVarDom domains (value ids 1 .. col_nvals - 1).
static int32_t tbatch_vuse(const ksim_handle* h, const ksim_pod& p, const PodPlan& pl, const ksim_topo_use* U) {
  if (!(pl.flags & kPlanPtab)) return -1;
  for (int32_t i = 0; i < p.use_count && i < KSIM_MAX_USES; i++) {
    const ksim_topo_use& u = U[i];
    if (u.kind != KSIM_USE_PTS_HARD) continue;
    if (!((pl.m.hard >> i) & 1u) || !((pl.m.ptab >> i) & 1u) || u.col == KSIM_COL_NONE || u.cls < 0) return -1;
    if (u.col >= (1 << (32 - kPlanVcolShift)) - 1) return -1;
    const int32_t nd = h->col_nvals[u.col] - 1;
    return nd >= 1 && nd <= kVarDom ? i : -1;
  }
  return -1;
}

// Topology batch runs (class 3 pods, ksim_tbatch.hip): tlen[i] = the number
// of consecutive class-3 pods from i (at most kTbPods) none of which reads a
// count class an earlier one of them adds through a use tbatch_conflict_ok
// refuses; cross[i]: the run crosses a conflict.  0 for the other pods.
// variants: a pod may also read such a class through its zone-variant use
// (tbatch_vuse) when exactly one earlier pod of the run adds the class and the
// use's column is the run's variant column vcol[i] (the first such use's;
// -1: none), so the chain names its slot by where that pod lands.
// uses: the queue's device use copies.
static void tbatch_runs(const ksim_pod_set* ps, const std::vector<ksim_topo_use>& uses,
                 const std::vector<uint8_t>& batchable, const std::vector<PodPlan>& plans, bool variants,
                 std::vector<int32_t>& tlen, std::vector<uint8_t>& cross, std::vector<int32_t>& vcol) {
  const int32_t n = ps->n_pods;
  tlen.assign((size_t)std::max(n, 0), 0);
  cross.assign((size_t)std::max(n, 0), 0);
  vcol.assign((size_t)std::max(n, 0), -1);
  int32_t n_cls = 0;
  for (int32_t k = 0; k < ps->n_adds; k++) n_cls = std::max(n_cls, ps->adds[k].cls + 1);
  std::vector<int32_t> stamp((size_t)n_cls, -1);   // class -> the window start that added it
  std::vector<int32_t> nadd((size_t)n_cls, 0);     // ... and how many pods of that run add it
  for (int32_t i = 0; i < n; i++) {
    if (batchable[i] != 3) continue;
    int32_t L = 0, vc = -1;
    bool crossed = false;
    for (int32_t j = i; j < n && L < kTbPods && batchable[j] == 3; j++, L++) {
      const ksim_pod& p = ps->pods[j];
      const ksim_topo_use* U = uses.data() + p.use_first;
      const int32_t vu = variants ? (int32_t)((plans[(size_t)j].flags >> kPlanVuseShift) & 31u) - 1 : -1;
      bool clash = false, hit = false;
      for (int32_t u = 0; u < p.use_count && !clash; u++) {
        const int32_t c = U[u].cls;
        if (c < 0 || c >= n_cls || stamp[c] != i) continue;
        hit = true;
        if (tbatch_conflict_ok(U[u])) continue;
        clash = !(u == vu && nadd[c] == 1 && (vc < 0 || vc == U[u].col));
        if (!clash) vc = U[u].col;
      }
      if (clash) break;
      crossed = crossed || hit;
      for (int32_t a = 0; a < p.add_count; a++) {
        const int32_t c = ps->adds[p.add_first + a].cls;
        if (stamp[c] != i) {
          stamp[c] = i;
          nadd[c] = 0;
        }
        nadd[c]++;   // per add entry: a pod listing the class twice counts as two adders
      }
    }
    tlen[i] = std::max(L, 1);
    cross[i] = crossed;
    vcol[i] = vc;
  }
}

int ksim_load_pods(ksim_handle* h, const ksim_pod_set* ps) {
  int rc = ensure_ready(h);
  if (rc) return rc;
  if (!ps || ps->n_pods < 0 || (ps->n_pods > 0 && !ps->pods) || ps->n_exprs < 0 || ps->n_terms < 0 ||
      ps->n_uses < 0 || ps->n_adds < 0 || ps->n_nn < 0)
    return set_err(h, KSIM_E_INVALID, "bad pod set");
  for (int32_t i = 0; i < ps->n_pods; i++)
    if ((rc = validate_pod(h, ps, i))) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  // The handle holds no queue until every buffer below is in place: a failure
  // part-way leaves it empty, never with pointers to freed or half-written
  // buffers (or graphs captured over them).
  h->dp = DevPods{};
  h->batchable.clear();
  // A queue with the same array sizes as the loaded one (a policy sweep
  // reloading its pods under each profile) is copied into the same buffers:
  // the device pointers, and so every captured graph, stay valid.  Every count
  // a graph captures by value (n_pods, n_exprs, n_terms, n_uses, n_adds,
  // n_nn) is a byte size over a fixed element size, so equal sizes mean equal
  // captured values.
  const size_t np1 = (size_t)std::max(ps->n_pods, 1);
  std::vector<ksim_topo_use> uses(ps->uses, ps->uses + std::max(ps->n_uses, 0));
  mark_unique(h, uses.data(), uses.size());
  PtabRegistry R;
  build_ptab(h, ps, uses, R);
  const std::vector<size_t> bytes = {sizeof(ksim_pod) * (size_t)ps->n_pods,
                                     sizeof(int4) * R.ent.size(), 4 * R.cfirst.size(), 4 * R.cidx.size(),
                                     8 * (size_t)R.len, sizeof(int4) * R.padd.size(),
                                     sizeof(ksim_label_expr) * (size_t)ps->n_exprs,
                                     sizeof(ksim_term) * (size_t)ps->n_terms,
                                     4 * (size_t)ps->n_nn,
                                     4 * np1,
                                     sizeof(ksim_topo_use) * (size_t)ps->n_uses,
                                     sizeof(PodPlan) * (size_t)ps->n_pods,
                                     sizeof(ksim_class_add) * (size_t)ps->n_adds,
                                     4 * np1, 4 * np1, 2 * np1, sizeof(PodReq) * ((size_t)kReqMaxClasses + 1)};
  const bool reuse = h->d_chosen && h->pod_buf_bytes == bytes;
  auto drop_queue = [&](int code) {
    drop_graphs(h);
    h->pod_bufs.clear();
    h->pod_buf_bytes.clear();
    h->d_chosen = nullptr;                         // in pod_bufs
    return code;
  };
  if (!reuse) drop_queue(KSIM_OK);
  size_t next_buf = 0;
  auto put = [&](auto*& dst, const void* src, size_t nbytes) -> int {
    if (!reuse) return h->pod_bufs.alloc(h, dst, nbytes, src);
    const DevBuf& b = h->pod_bufs[next_buf++];
    const hipError_t e = (src && nbytes) ? hipMemcpyAsync(b.p, src, nbytes, hipMemcpyHostToDevice, h->stream)
                                         : hipMemsetAsync(b.p, 0, b.bytes, h->stream);
    if (e != hipSuccess) return hip_fail(h, e, "pod upload");
    dst = (typename std::remove_reference<decltype(dst)>::type)b.p;
    return KSIM_OK;
  };
  std::vector<int32_t> bf(np1, 0);
  std::vector<uint8_t> batchable((size_t)ps->n_pods, 0);
  h->topo.assign((size_t)ps->n_pods, 0);
  h->xdom_len.assign((size_t)ps->n_pods, 0);
  h->trivial.assign((size_t)ps->n_pods, 0);
  h->noadd.assign((size_t)ps->n_pods, 0);
  h->noscalar.assign((size_t)ps->n_pods, 0);
  h->hard_small.assign((size_t)ps->n_pods, 1);
  h->soft_le1.assign((size_t)ps->n_pods, 1);
  h->xreg_len.assign((size_t)ps->n_pods, 0);
  // classes some pod of the queue adds to: an image use of one would not be
  // static (the encoders never emit that; a hand-built queue may)
  std::vector<uint8_t> added((size_t)std::max(h->dc.n_classes, 1), 0);
  for (int32_t k = 0; k < ps->n_adds; k++)
    if (ps->adds[k].cls >= 0 && ps->adds[k].cls < h->dc.n_classes) added[(size_t)ps->adds[k].cls] = 1;
  for (int32_t i = 0; i < ps->n_pods; i++) {
    bool nv = false;
    batchable[i] = (uint8_t)pod_batchable(h, ps->pods[i], ps->uses, &nv);
    if (batchable[i] && ps->pods[i].use_count == 1 && ps->uses[ps->pods[i].use_first].cls >= 0 &&
        added[(size_t)ps->uses[ps->pods[i].use_first].cls]) {
      batchable[i] = 0;
      nv = false;
    }
    if (nv) bf[i] |= kPodNormVaries;
    h->topo[i] = ps->pods[i].use_count > 0 ? (R.pod[i] ? 2 : 1) : 0;
    // sharded-cycle exchange sizes, laid out as k_dom_pack / k_window_sh do
    bool soft = false;
    int n_soft = 0;
    int64_t xr = 1;
    for (int32_t k = 0; k < ps->pods[i].use_count; k++) {
      const ksim_topo_use& u = ps->uses[ps->pods[i].use_first + k];
      if (use_needs_dom(u)) h->xdom_len[i] += h->col_nvals[u.col];
      if (u.kind == KSIM_USE_PTS_HARD && u.col != KSIM_COL_NONE && h->col_nvals[u.col] > kFuseMinValues) h->hard_small[i] = 0;
      if (use_registers_values(u)) {
        xr += h->col_nvals[u.col];
        bf[i] |= kPodRegistersValues;
      }
      soft = soft || u.kind == KSIM_USE_PTS_SOFT;
      n_soft += u.kind == KSIM_USE_PTS_SOFT ? 1 : 0;
    }
    h->soft_le1[i] = n_soft <= 1 ? 1 : 0;
    h->xreg_len[i] = soft ? xr : 0;
    // class-2 pods (pod_batchable) read full rows: taints, labels, scalar columns
    if (static_trivial(h, ps->pods[i]) && batchable[i] != 2) bf[i] |= kBatchStaticTrivial;
    h->trivial[i] = (bf[i] & kBatchStaticTrivial) ? 1 : 0;
    h->noadd[i] = ps->pods[i].add_count == 0 ? 1 : 0;
    h->noscalar[i] = (ps->pods[i].flags & KSIM_POD_HAS_SCALAR) == 0 ? 1 : 0;
  }
  // static classes (DevPods::stab): the batch pods without scalar requests
  // (trivial ones too, so a run mixing them with static-plugin pods takes
  // the STAB kernels)
  std::vector<int32_t> scls(np1, -1), srep(np1, 0);
  int32_t ncls = 0;
  {
    std::unordered_map<std::string, int32_t> ids;
    std::string sig;
    for (int32_t i = 0; i < ps->n_pods; i++) {
      const ksim_pod& q = ps->pods[i];
      if (batchable[i] != 1 && batchable[i] != 2) continue;
      if ((q.flags & KSIM_POD_HAS_SCALAR) || !stab_signature(ps, q, sig)) continue;
      auto it = ids.find(sig);
      if (it == ids.end()) {
        if (ncls >= kStabMaxClasses) continue;
        it = ids.emplace(sig, ncls).first;
        srep[(size_t)ncls++] = i;
      }
      scls[(size_t)i] = it->second;
    }
  }
  // request classes (ReqTab): the pods run_fast accepts, by their five request
  // fields (such pods request no scalar resources)
  std::vector<uint16_t> rcls(np1, 0xffff);
  std::vector<PodReq> rreq;
  {
    std::map<std::array<int64_t, 5>, int32_t> ids;
    for (int32_t i = 0; i < ps->n_pods; i++) {
      const ksim_pod& q = ps->pods[i];
      if (!h->trivial[i] || batchable[i] != 1 || (q.flags & KSIM_POD_HAS_SCALAR)) continue;
      const std::array<int64_t, 5> key = {q.req_cpu, q.req_mem, q.req_eph, q.nz_cpu, q.nz_mem};
      auto it = ids.find(key);
      if (it == ids.end()) {
        if ((int32_t)ids.size() > kReqMaxClasses) break;   // too many: no table for this queue
        it = ids.emplace(key, (int32_t)ids.size()).first;
        rreq.push_back(PodReq{key[0], key[1], key[2], key[3], key[4]});
      }
      rcls[(size_t)i] = (uint16_t)it->second;
    }
  }
  const int32_t n_rcls = (int32_t)rreq.size();       // kReqMaxClasses + 1: too many
  rreq.resize((size_t)kReqMaxClasses + 1, PodReq{0, 0, 0, 0, 0});
  std::vector<PodPlan> plans((size_t)ps->n_pods);
  for (int32_t i = 0; i < ps->n_pods; i++) {
    plans[i] = make_plan(h, ps->pods[i], uses.data() + std::max(ps->pods[i].use_first, 0));
    if (R.pod[i]) {
      plans[i].flags |= kPlanPtab;
      plans[i].m.ptab = R.mask[i];
    }
    if (!R.padd_first.empty()) {   // the table updates of its binds, listed
      plans[i].flags |= kPlanTadds;
      plans[i].tadd_first = R.padd_first[(size_t)i];
      plans[i].tadd_count = R.padd_count[(size_t)i];
    }
    if (batchable[i] == 0 && tbatch_admit(h, ps->pods[i], plans[i], h->hard_small[i] != 0, h->soft_le1[i] != 0)) {
      batchable[i] = 3;
      bf[i] |= kPodTopoBatch;
      const int32_t vu = tbatch_vuse(h, ps->pods[i], plans[i], uses.data() + std::max(ps->pods[i].use_first, 0));
      if (vu >= 0) plans[i].flags |= (uint32_t)(vu + 1) << kPlanVuseShift;
    }
  }
  std::vector<uint8_t> tcross, c2;
  std::vector<int32_t> tvcol, v2;
  tbatch_runs(ps, uses, batchable, plans, !ab(kAbTbVar), h->tlen, tcross, tvcol);
  tbatch_runs(ps, uses, batchable, plans, false, h->tlen_plain, c2, v2);   // replicated handles
  for (int32_t i = 0; i < ps->n_pods; i++) {
    // a run crosses with variants when it does without (a prefix of it)
    bf[i] |= (std::min(h->tlen[i], kTlenMask) << kTlenShift) | (std::min(h->tlen_plain[i], kTlenMask) << kTlenPlainShift) |
             (tcross[(size_t)i] ? kPodTbCross : 0);
    plans[i].flags |= (uint32_t)(tvcol[(size_t)i] + 1) << kPlanVcolShift;
  }
  DevPods P{};
  if ((rc = put(P.pods, ps->pods, sizeof(ksim_pod) * ps->n_pods)) ||
      (rc = put(P.exprs, ps->exprs, sizeof(ksim_label_expr) * ps->n_exprs)) ||
      (rc = put(P.terms, ps->terms, sizeof(ksim_term) * ps->n_terms)) ||
      (rc = put(P.nn, ps->nn, 4 * (size_t)ps->n_nn)) ||
      (rc = put(P.bflags, bf.data(), 4 * bf.size())) ||
      (rc = put(P.uses, uses.data(), sizeof(ksim_topo_use) * uses.size())) ||
      (rc = put(P.plans, plans.data(), sizeof(PodPlan) * plans.size())) ||
      (rc = put(P.adds, ps->adds, sizeof(ksim_class_add) * (size_t)ps->n_adds)) ||
      (rc = put(h->d_sclass, scls.data(), 4 * np1)) ||
      (rc = put(h->d_srep, srep.data(), 4 * np1)))
    return drop_queue(rc);
  h->stab_ncls = ncls;
  h->sclass.assign(scls.begin(), scls.begin() + ps->n_pods);
  h->stab_dirty = true;
  h->d_rcls = nullptr;
  h->rq_ncls = 0;
  uint16_t* d_rcls = nullptr;
  if ((rc = put(d_rcls, rcls.data(), 2 * np1)) ||
      (rc = put(h->d_rreq, rreq.data(), sizeof(PodReq) * rreq.size())))
    return drop_queue(rc);
  h->d_rcls = d_rcls;
  h->rq_cls.assign(rcls.begin(), rcls.begin() + ps->n_pods);
  h->rq_ncls = n_rcls;
  if ((rc = put(P.ptab_ent, R.ent.data(), sizeof(int4) * R.ent.size())) ||
      (rc = put(P.ptab_cfirst, R.cfirst.data(), 4 * R.cfirst.size())) ||
      (rc = put(P.ptab_cidx, R.cidx.data(), 4 * R.cidx.size())) ||
      (rc = put(P.ptab, nullptr, 8 * (size_t)R.len)) ||   // filled by k_ptab_init
      (rc = put(P.ptab_padd, R.padd.data(), sizeof(int4) * R.padd.size())))
    return drop_queue(rc);
  if (R.cfirst.empty()) P.ptab_cfirst = nullptr;
  P.n_ptab = (int32_t)R.ent.size();
  P.n_uses = ps->n_uses;
  P.n_adds = ps->n_adds;
  P.n_nn = ps->n_nn;
  P.n_pods = ps->n_pods;
  P.n_exprs = ps->n_exprs;
  P.n_terms = ps->n_terms;
  hipError_t e = hipSuccess;
  if (!reuse) {                                    // behind the arrays put() reuses by position
    if ((rc = h->pod_bufs.alloc(h, h->d_chosen, 4 * np1))) return drop_queue(rc);
    h->pod_buf_bytes = bytes;
  }
  if ((e = hipMemsetAsync(h->d_chosen, 0xff, 4 * np1, h->stream)) != hipSuccess ||
      (e = hipStreamSynchronize(h->stream)) != hipSuccess)
    return drop_queue(hip_fail(h, e, "pod queue setup"));
  h->batchable = std::move(batchable);
  h->dp = P;
  launch_ptab_init(h->dc, P, h->stream);
  if ((e = hipGetLastError()) != hipSuccess || (e = hipStreamSynchronize(h->stream)) != hipSuccess) {
    h->dp = DevPods{};
    return drop_queue(hip_fail(h, e, "persistent tables"));
  }
  return KSIM_OK;
}

int ksim_schedule_loaded(ksim_handle* h, int32_t first, int32_t count, int32_t* chosen, ksim_batch_stats* stats) {
  int rc = ensure_ready(h);
  if (rc) return rc;
  if (!h->dp.pods && count > 0) return set_err(h, KSIM_E_INVALID, "no pods loaded");
  if (first < 0 || count < 0 || first + count > h->dp.n_pods) return set_err(h, KSIM_E_INVALID, "range out of loaded pods");
  HIPCHK(h, hipSetDevice(h->device));
  if ((rc = ensure_stab(h))) return rc;
  // the counters start from zero: an unsharded call's first run zeroes them
  // (run_range; a deferred-commit run does it in its begin launch)
  const bool defer_zero = !is_sharded(h) && count > 0;
  if (!defer_zero && (rc = reset_counters(h, h->stream))) return rc;
  int64_t perpod = 0;
  HIPCHK(h, hipEventRecord(h->ev0, h->stream));
  if (is_sharded(h)) {
    for (int32_t i = first; i < first + count; i++) perpod += pod_on_batch(h, i) ? 0 : 1;
    rc = shard_schedule({h}, first, count);
  } else {
    h->counters_pending = defer_zero;
    rc = for_each_run(h, first, count, [&](int32_t a, int32_t b, bool batch, bool topo) {
      if (!batch) perpod += b - a;
      return run_range(h, a, b, plan_run(h, a, b, batch, topo));
    });
    h->counters_pending = false;
  }
  if (rc) return rc;
  HIPCHK(h, hipEventRecord(h->ev1, h->stream));
  HIPCHK(h, hipEventSynchronize(h->ev1));
  HIPCHK(h, hipGetLastError());
  if (chosen && count) HIPCHK(h, hcopy(h, chosen, h->d_chosen + first, 4 * (size_t)count, hipMemcpyDeviceToHost));
  if (stats) {
    DevState st;
    if ((rc = read_state(h, st))) return rc;
    float ms = 0;
    HIPCHK(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
    stats->pods = count;
    stats->scheduled = st.scheduled;
    stats->unschedulable = st.unschedulable;
    stats->evals = st.evals;
    stats->device_ms = ms;
    stats->batches = st.batches;
    stats->truncations = st.truncations;
    stats->perpod_cycles = perpod;
  }
  return KSIM_OK;
}

int ksim_sweep_loaded(ksim_handle* h, int32_t first, int32_t count, const ksim_profile* profs, int32_t n_profs,
                      int32_t max_lanes, int32_t* chosen, ksim_batch_stats* stats) {
  int rc = ensure_ready(h);
  if (rc) return rc;
  if (!profs || n_profs < 1) return set_err(h, KSIM_E_INVALID, "sweep: no profiles");
  if (!h->dp.pods && count > 0) return set_err(h, KSIM_E_INVALID, "no pods loaded");
  if (first < 0 || count < 0 || first + count > h->dp.n_pods) return set_err(h, KSIM_E_INVALID, "range out of loaded pods");
  if (!chosen && count > 0) return set_err(h, KSIM_E_INVALID, "sweep: chosen is null");
  if (max_lanes < 0 || max_lanes > KSIM_SWEEP_MAX_LANES)
    return set_err(h, KSIM_E_INVALID, "sweep: max_lanes outside [0, " + std::to_string(KSIM_SWEEP_MAX_LANES) + "]");
  static_assert(KSIM_SWEEP_MAX_LANES == kSweepMaxLanes && KSIM_SWEEP_DEFAULT_LANES <= kSweepMaxLanes, "sweep lanes");
  for (int32_t v = 0; v < n_profs; v++)
    if ((rc = validate_profile(h, &profs[v]))) return rc;
  // ---- the packed path's conditions -------------------------------------------
  auto no = [&](const std::string& why) { return set_err(h, KSIM_E_UNSUPPORTED, "packed sweep: " + why); };
  if (!lazy_enabled()) return no("this library runs the three-launch batches (A/B flavor)");
  if (is_sharded(h) || h->replicated) return no("the handle is sharded or replicated");
  if (adapt_mode(h)) return no("the profile scores a window of the nodes (ADAPT); percentageOfNodesToScore must keep every node");
  if (h->dc.n > kKeepPerLane * 1024)
    return no("the cluster has more than " + std::to_string(kKeepPerLane * 1024) + " nodes");
  for (int32_t v = 0; v < n_profs; v++) {
    ksim_profile q = profs[v];
    std::memcpy(q.score_weight, h->prof.score_weight, sizeof(q.score_weight));
    if (std::memcmp(&q, &h->prof, sizeof(q)) != 0)
      return no("profile " + std::to_string(v) + " differs from the handle's in more than score_weight");
  }
  {
    // one run of the deferred-commit FAST batches under the handle's profile
    int32_t runs = 0;
    bool one = true;
    (void)for_each_run(h, first, count, [&](int32_t a, int32_t b, bool batch, bool topo) {
      runs++;
      const RunPlan p = plan_run(h, a, b, batch, topo);
      one = one && p.form == RunForm::kLazy && p.fast && !p.stab;
      return KSIM_OK;
    });
    if (runs > 1 || !one) return no("the range is not one run of the deferred-commit FAST batches");
  }
  std::vector<BatchProg> bps((size_t)n_profs);
  for (int32_t v = 0; v < n_profs; v++) {
    bps[(size_t)v] = compile_batch_prog(&profs[v]);
    const BatchProg& bp = bps[(size_t)v];
    // pod_batchable under vector v: the run's pods are class 1 under the
    // handle's profile (run_fast), so no normalized score of theirs varies
    // over nodes (a property of the plugin lists and the pods, which the
    // vectors share), and the class reads the weights in one test only
    if ((int64_t)kMaxNodeScore * (bp.w_fit + bp.w_ba) >= kKeyTotalLimit)
      return no("profile " + std::to_string(v) + ": totals past the batch key's range (its pods take the per-pod path)");
    if (fast_def(bp) != fast_def(bps[0])) return no("the vectors give the FAST key different shapes");
  }
  if (count == 0) {
    if (stats) std::memset(stats, 0, sizeof(ksim_batch_stats) * (size_t)n_profs);
    return KSIM_OK;
  }
  HIPCHK(h, hipSetDevice(h->device));
  const int32_t lanes = std::min(max_lanes ? max_lanes : KSIM_SWEEP_DEFAULT_LANES, n_profs);
  // the vectors' device copies: [n_profs] ksim_profile, then [n_profs] BatchProg
  const size_t pbytes = (sizeof(ksim_profile) * (size_t)n_profs + 255) & ~(size_t)255;
  if ((rc = h->sweep_profs.reserve(h, pbytes + sizeof(BatchProg) * (size_t)n_profs, Idle::kSync))) return rc;
  ksim_profile* d_profs = (ksim_profile*)h->sweep_profs.p;
  BatchProg* d_bps = (BatchProg*)((char*)h->sweep_profs.p + pbytes);
  HIPCHK(h, hipEventRecord(h->ev0, h->stream));
  HIPCHK(h, hipMemcpyAsync(d_profs, profs, sizeof(ksim_profile) * (size_t)n_profs, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(d_bps, bps.data(), sizeof(BatchProg) * (size_t)n_profs, hipMemcpyHostToDevice, h->stream));
  if ((rc = run_sweep(h, first, first + count, n_profs, lanes, fast_def(bps[0]), d_profs, d_bps, chosen, stats))) {
    (void)hipStreamSynchronize(h->stream);         // nothing in flight reads the caller's or this frame's memory
    return rc;
  }
  HIPCHK(h, hipEventRecord(h->ev1, h->stream));
  HIPCHK(h, hipEventSynchronize(h->ev1));
  HIPCHK(h, hipGetLastError());
  if (stats) {
    float ms = 0;
    HIPCHK(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
    for (int32_t v = 0; v < n_profs; v++) stats[v].device_ms = ms;
  }
  return KSIM_OK;
}

int ksim_set_shard(ksim_handle* h, int32_t node_base, int32_t n_total) {
  if (const int prc = flush_pend_bind(h)) return prc;   // a queued Reserve lands first
  if (!h) return KSIM_E_INVALID;
  h->stab_dirty = true;
  if (node_base < 0 || n_total < 0 || n_total > KSIM_MAX_NODES || node_base > n_total)
    return set_err(h, KSIM_E_INVALID, "bad shard range");
  if (h->has_cluster) return set_err(h, KSIM_E_INVALID, "ksim_set_shard must precede ksim_set_cluster");
  h->shard_base = node_base;
  h->shard_total = n_total;
  return KSIM_OK;
}

int ksim_set_eval_range(ksim_handle* h, int32_t eval_lo, int32_t eval_hi) {
  if (const int prc = flush_pend_bind(h)) return prc;   // a queued Reserve lands first
  if (!h) return KSIM_E_INVALID;
  if (!h->has_cluster) return set_err(h, KSIM_E_INVALID, "ksim_set_eval_range needs the cluster (ksim_set_cluster)");
  if (h->shard_total != 0) return set_err(h, KSIM_E_INVALID, "a node-shard handle holds only its nodes: no eval range");
  if (h->dc.vol_nf) return set_err(h, KSIM_E_UNSUPPORTED, "a handle with a volume table (ksim_set_volume_limits) cannot be replicated");
  if (eval_lo < 0 || eval_hi < eval_lo || eval_hi > h->dc.n) return set_err(h, KSIM_E_INVALID, "bad eval range");
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  drop_cycle_graphs(h);                        // shard batch graphs captured with the old range
  h->replicated = true;
  h->eval_lo = eval_lo;
  h->eval_hi = eval_hi;
  return KSIM_OK;
}

int ksim_comm_unique_id(uint8_t* id) {
  if (!id) return KSIM_E_INVALID;
  if (!rccl().ok) return KSIM_E_RCCL;
  ncclUniqueId u;
  if (rccl().get_unique_id(&u) != ncclSuccess) return KSIM_E_RCCL;
  std::memcpy(id, u.internal, KSIM_COMM_ID_BYTES);
  return KSIM_OK;
}

int ksim_comm_init(ksim_handle* h, int32_t rank, int32_t world, const uint8_t* id) {
  if (const int prc = flush_pend_bind(h)) return prc;   // a queued Reserve lands first
  if (!h || !id) return KSIM_E_INVALID;
  if (world < 1 || world > kMaxShards || rank < 0 || rank >= world)
    return set_err(h, KSIM_E_INVALID, "world must be 1.." + std::to_string(kMaxShards));
  if (h->has_cluster && h->dc.vol_nf)
    return set_err(h, KSIM_E_UNSUPPORTED, "a handle with a volume table (ksim_set_volume_limits) cannot join a group");
  if (!rccl().ok) return set_err(h, KSIM_E_RCCL, "librccl not found");
  HIPCHK(h, hipSetDevice(h->device));
  if (h->comm) (void)rccl().comm_destroy(h->comm);
  h->comm = nullptr;
  ncclUniqueId u;
  std::memcpy(u.internal, id, KSIM_COMM_ID_BYTES);
  const ncclResult_t r = rccl().comm_init_rank(&h->comm, world, u, rank);
  if (r != ncclSuccess) {
    h->comm = nullptr;
    return set_err(h, KSIM_E_RCCL, std::string("ncclCommInitRank: ") + rccl().error_string(r));
  }
  h->rank = rank;
  h->world = world;
  if (h->rep_primary != (rank == 0)) {
    drop_graphs(h);                        // captured with the other counting flag
    h->rep_primary = rank == 0;
  }
  return KSIM_OK;
}

int ksim_group_schedule_loaded(ksim_handle** hs, int32_t n, int32_t first, int32_t count, int32_t* chosen,
                               ksim_batch_stats* stats) {
  if (!hs || n < 1 || n > kMaxShards) return KSIM_E_INVALID;
  ksim_handle* h0 = hs[0];
  std::vector<ksim_handle*> v(hs, hs + n);
  int32_t expect = 0;
  for (auto* h : v) {
    int rc = ensure_ready(h);
    if (rc) return rc;
    if (h->comm) return set_err(h0, KSIM_E_INVALID, "group handles must not hold a communicator");
    if (h->device != h0->device) return set_err(h0, KSIM_E_INVALID, "group handles must share one device");
    if (!h->dp.pods || h->dp.n_pods != h0->dp.n_pods) return set_err(h0, KSIM_E_INVALID, "pods not loaded alike");
    if (h->replicated != h0->replicated) return set_err(h0, KSIM_E_INVALID, "mixed replicated / shard handles");
    if (h->replicated) {                       // replicas: whole clusters, eval ranges tiling it in order
      if (h->dc.n != h0->dc.n || h->eval_lo != expect)
        return set_err(h0, KSIM_E_INVALID, "eval ranges must tile the cluster in order");
      expect = h->eval_hi;
      if (h->rep_primary != (h == h0)) {       // the first replica counts whole-run evaluations
        (void)hipStreamSynchronize(h->stream);
        drop_graphs(h);
        h->rep_primary = h == h0;
      }
      continue;
    }
    if (h->dc.n_total != h0->dc.n_total || h->dc.base != expect)
      return set_err(h0, KSIM_E_INVALID, "shards must tile the cluster in order");
    expect += h->dc.n;
  }
  if (expect != h0->dc.n_total) return set_err(h0, KSIM_E_INVALID, "shards must tile the cluster");
  if (first < 0 || count < 0 || first + count > h0->dp.n_pods) return set_err(h0, KSIM_E_INVALID, "range out of loaded pods");
  HIPCHK(h0, hipSetDevice(h0->device));
  int rc;
  for (auto* h : v)
    if ((rc = ensure_stab(h)) || (rc = reset_counters(h, h->stream))) return rc;
  HIPCHK(h0, hipEventRecord(h0->ev0, h0->stream));
  if (count && (rc = shard_schedule(v, first, count))) return rc;
  HIPCHK(h0, hipEventRecord(h0->ev1, h0->stream));
  HIPCHK(h0, hipEventSynchronize(h0->ev1));
  if (chosen && count) HIPCHK(h0, hcopy(h0, chosen, h0->d_chosen + first, 4 * (size_t)count, hipMemcpyDeviceToHost));
  if (stats) {
    std::memset(stats, 0, sizeof(*stats));
    for (auto* h : v) {
      DevState st;
      if ((rc = read_state(h, st))) return rc;
      stats->evals += st.evals;                // each shard counts its own nodes
      if (h == h0) {
        stats->scheduled = st.scheduled;
        stats->unschedulable = st.unschedulable;
        stats->batches = st.batches;
        stats->truncations = st.truncations;
      }
    }
    float ms = 0;
    HIPCHK(h0, hipEventElapsedTime(&ms, h0->ev0, h0->ev1));
    stats->pods = count;
    stats->device_ms = ms;
    // as ksim_schedule_loaded on a sharded handle: the pods the group's runs took off the batch path
    for (int32_t i = first; i < first + count; i++) stats->perpod_cycles += pod_on_batch(h0, i) ? 0 : 1;
  }
  return KSIM_OK;
}

int ksim_schedule_batch(ksim_handle* h, const ksim_pod_set* ps, int32_t* chosen, ksim_batch_stats* stats) {
  int rc = ksim_load_pods(h, ps);
  if (rc) return rc;
  return ksim_schedule_loaded(h, 0, ps->n_pods, chosen, stats);
}

// ksim_time_kernels' slots: the kernels of the six launch forms, a family per
// RunForm in the forms' order, each family's kernels in launch order.  A slot
// is its family's base plus the kernel's place in it (ksim_kernel_name).
struct KernelFamily { const char* const* names; int count; };
constexpr KernelFamily kFamilies[] = {
    {kKernelNames, kKernelsPerCycle},       {kBatchKernelNames, kKernelsPerBatch},
    {kAdaptKernelNames, kKernelsPerAdapt},  {kTbatchKernelNames, kKernelsPerTbatch},
    {kLazyKernelNames, kKernelsPerLazy},    {kLazyAdaptKernelNames, kKernelsPerLazyAdapt},
};
constexpr int kFamilyCount = (int)(sizeof(kFamilies) / sizeof(kFamilies[0]));
static_assert(kFamilyCount == (int)RunForm::kLazyAdapt + 1, "a kernel family per run form");
constexpr int family_base(int f) { return f == 0 ? 0 : family_base(f - 1) + kFamilies[f - 1].count; }
constexpr int kKernelSlots = family_base(kFamilyCount);

int ksim_time_eval(ksim_handle* h, int32_t first, int32_t reps, double* avg_ms, int32_t* kernel) {
  int rc = ensure_ready(h);
  if (rc) return rc;
  if (!avg_ms || reps < 1 || !h->dp.pods || first < 0 || first >= h->dp.n_pods)
    return set_err(h, KSIM_E_INVALID, "bad ksim_time_eval arguments");
  const bool batch = pod_on_batch(h, first) && !is_sharded(h);
  if (batch && h->batchable[first] == 3)
    return set_err(h, KSIM_E_UNSUPPORTED, "topology batch evaluations span two kernels");
  if (batch && adapt_mode(h)) return set_err(h, KSIM_E_UNSUPPORTED, "ADAPT batch evaluations span two kernels");
  HIPCHK(h, hipSetDevice(h->device));
  if ((rc = ensure_stab(h))) return rc;
  // two batches' pods: the deferred-commit timing below keys batch 1 (a full
  // batch whatever batch 0 commits)
  const int32_t end = batch ? std::min(h->dp.n_pods, first + 2 * kBatchPods) : first + 1;
  if ((rc = set_run(h, first, end))) return rc;
  const RunPlan plan = plan_run(h, first, end, batch, !batch && h->topo[first] != 0);
  LaunchArgs a = make_args(h, h->dp, h->d_chosen);
  apply_plan(plan, a);
  // one warming launch (code object, caches), then `reps` back to back
  auto timed = [&](auto&& launch) -> int {
    launch();
    HIPCHK(h, hipEventRecord(h->ev0, h->stream));
    for (int32_t i = 0; i < reps; i++) launch();
    HIPCHK(h, hipEventRecord(h->ev1, h->stream));
    HIPCHK(h, hipEventSynchronize(h->ev1));
    HIPCHK(h, hipGetLastError());
    float ms = 0;
    HIPCHK(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
    *avg_ms = ms / reps;
    return KSIM_OK;
  };
  if (plan.form == RunForm::kLazy) {
    // the deferred-commit evaluation launch as the run issues it: batch 0 of
    // the run (both launches), then batch 1's k_batch_top_commit repeated
    // (idempotent: it reads X[0], st[0] and slot 0, and writes X[1], st[1],
    // the lists and batch 0's placements); the handle's own buffers keep
    // their contents
    // (the one departure from the plan: with the request-class table when the
    // run from `first` to the queue's end takes it, not the two batches timed
    // here: the launch the timing stands for)
    if ((rc = lazy_begin(h))) return rc;
    const bool rt = reqtab_ok(h, first, h->dp.n_pods);
    if (rt && (rc = reqtab_begin(h, a, first, end))) return rc;
    launch_batch_lazy(lazy_batch(h, a, 0, rt), h->stream);
    const LazyBatch z = lazy_batch(h, a, 1, rt);
    if ((rc = timed([&] { launch_lazy_top(z, h->stream); }))) return rc;
    if (kernel) *kernel = family_base(plan.family());   // k_batch_top_commit
    return KSIM_OK;
  }
  rc = timed([&] {
    if (batch) launch_batch_eval_only(a, h->stream);
    else launch_filter_only(a, h->stream);
  });
  if (rc) return rc;
  // the timed no-window filter passes added into the window counters
  if (!batch) HIPCHK(h, hzero(h, h->sc.win, sizeof(WinState)));
  if (kernel) *kernel = family_base(plan.family()) + (batch ? 0 : 2);   // k_batch_top / k_filter_score
  return KSIM_OK;
}

const char* ksim_kernel_name(int32_t k) {
  for (int f = 0; f < kFamilyCount; f++)
    if (k >= family_base(f) && k < family_base(f + 1)) return kFamilies[f].names[k - family_base(f)];
  return nullptr;
}

// One timed stretch of ksim_time_kernels: `iters` iterations of `per` kernels,
// launch(evs) recording its per + 1 events and returning the mask of the
// kernels it launched; then read(), the caller's state read, and did(), the
// iterations that did work by that state, whose times go to sum / n from slot
// 0 up.  The events are destroyed on every path.
template <class L, class R, class D>
int timed_stretch(ksim_handle* h, int32_t iters, int per, double* sum, int64_t* n, L&& launch, R&& read, D&& did) {
  std::vector<hipEvent_t> evs((size_t)iters * (per + 1), nullptr);
  const int rc = [&]() -> int {
    for (auto& e : evs) HIPCHK(h, hipEventCreate(&e));
    uint32_t launched = 0;
    for (int32_t t = 0; t < iters; t++) launched = launch(&evs[(size_t)t * (per + 1)]);
    HIPCHK(h, hipGetLastError());
    if (int r = read()) return r;
    const int32_t worked = did();
    for (int32_t t = 0; t < worked; t++)
      for (int k = 0; k < per; k++) {
        if (!((launched >> k) & 1u)) continue;     // an empty event pair, not a kernel
        float ms = 0;
        HIPCHK(h, hipEventElapsedTime(&ms, evs[(size_t)t * (per + 1) + k], evs[(size_t)t * (per + 1) + k + 1]));
        sum[k] += ms;
        n[k] += 1;
      }
    return KSIM_OK;
  }();
  for (auto& e : evs)
    if (e) (void)hipEventDestroy(e);
  return rc;
}

int ksim_time_kernels(ksim_handle* h, int32_t first, int32_t count, double* avg_ms, int64_t* launches, int32_t cap) {
  int rc = ensure_ready(h);
  if (rc) return rc;
  if (!avg_ms || cap < kKernelSlots) return set_err(h, KSIM_E_INVALID, "avg_ms too small");
  if (!h->dp.pods || first < 0 || count <= 0 || first + count > h->dp.n_pods)
    return set_err(h, KSIM_E_INVALID, "range out of loaded pods");
  HIPCHK(h, hipSetDevice(h->device));
  if ((rc = ensure_stab(h))) return rc;
  double sum[kKernelSlots] = {0};
  int64_t n[kKernelSlots] = {0};
  LaunchArgs a = make_args(h, h->dp, h->d_chosen);
  rc = for_each_run(h, first, count, [&](int32_t lo, int32_t hi, bool batch, bool topo) -> int {
    int r;
    if ((r = set_run(h, lo, hi))) return r;
    // the kernel variants the run itself launches: its plan
    const RunPlan plan = plan_run(h, lo, hi, batch, topo);
    apply_plan(plan, a);
    const int per = kFamilies[plan.family()].count, base = family_base(plan.family());
    int32_t cursor = lo;
    DevState st;
    if (plan.lazy()) {
      // deferred-commit batches: two (P100) or three to four (ADAPT) launches
      // each, a flush (untimed) before every state read
      HIPCHK(h, hipMemsetAsync(&h->st->batches, 0, 4, h->stream));
      if ((r = lazy_begin(h))) return r;
      if (plan.rt && (r = reqtab_begin(h, a, lo, hi))) return r;
      int64_t i = 0;
      int32_t done_batches = 0;
      while (cursor < hi) {
        const int32_t iters = std::min(64, (hi - cursor + kBatchPods - 1) / kBatchPods);
        r = timed_stretch(
            h, iters, per, sum + base, n + base,
            [&](hipEvent_t* evs) { return lazy_launch(h, lazy_batch(h, a, i++, plan.rt), h->stream, evs); },
            [&]() -> int {
              lazy_flush(h, lazy_batch(h, a, i, plan.rt), h->stream);
              HIPCHK(h, hipGetLastError());
              return read_state_at(h, (i & 1) ? h->lazy.st1 : h->st, st);
            },
            [&] { return std::min<int32_t>(iters, st.batches - done_batches); });
        if (r) return r;
        done_batches = st.batches;
        if (st.cursor <= cursor) return set_err(h, KSIM_E_DEVICE, "no progress while timing");
        cursor = st.cursor;
        i++;
      }
      return lazy_end(h, i - 1);
    }
    const bool tb = plan.form == RunForm::kTbatch;
    if (tb && (r = tbatch_begin(h))) return r;
    while (cursor < hi) {
      int32_t iters = batch ? std::min(64, (hi - cursor + kBatchPods - 1) / kBatchPods) : std::min(512, hi - cursor);
      if (tb) {                                  // the batches the host's run lengths predict (run_tbatch)
        iters = 0;
        for (int32_t i = cursor; i < hi && iters < 64; iters++) i += std::min(std::min(kTbPods, hi - i), std::max(h->tlen[i], 1));
      }
      if (batch) HIPCHK(h, hipMemsetAsync(&h->st->batches, 0, 4, h->stream));
      r = timed_stretch(
          h, iters, per, sum + base, n + base,
          [&](hipEvent_t* evs) {
            return tb             ? launch_tbatch(a, h->stream, evs)
                   : plan.adapt() ? launch_batch_adapt(a, h->stream, evs)
                   : batch        ? launch_batch(a, h->stream, evs)
                                  : launch_cycle(a, h->stream, false, topo, evs);
          },
          [&] { return read_state(h, st); },
          // iterations past the end exit at once; count only those that did work
          [&] { return batch ? std::min<int32_t>(iters, st.batches) : std::min(iters, st.cursor - cursor); });
      if (r) return r;
      if (st.cursor <= cursor) return set_err(h, KSIM_E_DEVICE, "no progress while timing");
      cursor = st.cursor;
    }
    return KSIM_OK;
  });
  if (rc) return rc;
  for (int k = 0; k < kKernelSlots; k++) {
    avg_ms[k] = n[k] ? sum[k] / n[k] : 0.0;
    if (launches) launches[k] = n[k];
  }
  return kKernelSlots;
}

extern "C" int ksim_get_diag(ksim_handle* h, int64_t* out, int32_t n) {
  if (!h || !out || n < 0) return KSIM_E_INVALID;
  DevState st;
  int rc = read_state(h, st);
  if (rc) return rc;
  int64_t v[3 + 16 + 2 + 4 + 3 + 5 + 2 + 3] = {st.batches, st.truncations, st.cuts};
  if (h->has_cluster) HIPCHK(h, hcopy(h, v + 3, h->sc.dbg, 8 * 16, hipMemcpyDeviceToHost));
  if (unsigned long long* cp = cp_clock_buffer())   // KSIM_CP_CLOCKS builds: the chain + pairs phase clocks
    HIPCHK(h, hcopy(h, v + 3, cp, 8 * 8, hipMemcpyDeviceToHost));
  if (unsigned long long* ad = adapt_dbg_buffer())  // KSIM_ADAPT_DBG builds: ADAPT batch ends
    HIPCHK(h, hcopy(h, v + 3, ad, 8 * 8, hipMemcpyDeviceToHost));
  v[19] = h->graph_captures;
  v[20] = h->match_ns;
  for (int k = 0; k < 4; k++) v[21 + k] = h->fw_counts[k];
  v[25] = (int64_t)batch_variant_reach();
  if (h->has_cluster && h->sc.tb_vpods) HIPCHK(h, hcopy(h, v + 26, h->sc.tb_vpods, 8, hipMemcpyDeviceToHost));
  v[27] = h->rtab_runs;
  v[28] = h->feed_syncs;
  v[29] = h->feed_past_end;
  v[30] = h->feed_fallbacks;
  v[31] = h->feed_topups;
  v[32] = h->feed_odd_ends;
  v[33] = st.stretches;
  v[34] = st.stretch_pods;
  v[35] = h->many_rows;
  v[36] = h->many_single;
  v[37] = h->many_dom_answered;
  const int32_t m = n < 38 ? n : 38;
  for (int32_t i = 0; i < m; i++) out[i] = v[i];
  return m;
}

extern "C" int32_t ksim_feed_more_batches(int32_t left, int32_t pending) {
  return lazy_more_batches(left, pending, kBatchPods);
}

extern "C" int ksim_batch_geometry(int32_t* out, int32_t n) {
  if (!out || n < 0) return KSIM_E_INVALID;
  const int32_t v[4] = {kBatchPods, kTopT, kTopThreads, kTileCand};
  const int32_t m = n < 4 ? n : 4;
  for (int32_t i = 0; i < m; i++) out[i] = v[i];
  return m;
}
