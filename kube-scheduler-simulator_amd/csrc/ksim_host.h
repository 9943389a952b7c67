// ksim_host.h — what the host runtime's units share: the handle behind the C
// ABI and the helpers ksim_engine.cpp defines for ksim_snapshot.cpp (the node
// snapshot's life cycle) and ksim_preempt_host.cpp (DefaultPreemption, term
// matching).  Private to csrc/: no device code includes it.
#pragma once

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <array>
#include <map>
#include <string>
#include <tuple>
#include <vector>

#include "ksim_internal.h"
#include "ksim_mem.h"

using namespace ksim;

// One pod (re-based) as a device pod set of its own, packed the way it is
// uploaded: every piece at a 64-byte aligned offset of one blob.
struct PodBlob {
  std::vector<char> bytes;
  size_t off[8];
  int32_t n_nn, n_exprs, n_terms, n_uses, n_adds;
};

// What a shard-group graph holds (ksim_engine.cpp group_graph): its protocol
// and the launch arguments that protocol bakes into the graph.
enum class GroupGraphKind : int32_t {
  kPerPod,       // kGraphCycles per-pod cycles: topo, xdom, xreg (the exchange lengths)
  kBatch,        // kGraphBatches P100 batches: fast
  kAdaptBatch,   // kGraphBatches ADAPT batches: fast
  kLazyBatch,    // kGraphBatches replicated deferred-commit batches
};

struct GroupGraphKey {
  GroupGraphKind kind = GroupGraphKind::kPerPod;
  bool topo = false, fast = false;
  int64_t xdom = 0, xreg = 0;
  bool operator<(const GroupGraphKey& o) const {
    return std::tie(kind, topo, fast, xdom, xreg) < std::tie(o.kind, o.topo, o.fast, o.xdom, o.xreg);
  }
};

// What a single handle's graph holds (ksim_engine.cpp handle_graph): its kind
// and, in arg, exactly the launch arguments that kind bakes into the graph.
enum class GraphKind : int32_t {
  kCycle,    // kGraphCycles per-pod cycles: {topo, fuse_min, fuse_ext, ptab}
  kBatch,    // kGraphBatches three-launch batches (P100 or ADAPT, by the profile): {fast, stab}
  kTbatch,   // kGraphBatches topology batches: {}
  kLazy,     // deferred-commit batches: {ADAPT, the request-class count (0: no table), tail}; the tail
             // graph is kLazySlots batches (run_lazy's top-ups), the whole one kGraphBatches
  kSweep,    // kGraphBatches packed sweep batches: {lanes, def}
};

struct GraphKey {
  GraphKind kind;
  std::array<int32_t, 4> arg;
  bool operator<(const GraphKey& o) const { return std::tie(kind, arg) < std::tie(o.kind, o.arg); }
};

// State of the handle that is dropped together lives together: a pool, the
// typed views into it and its sizes in one struct, dropped by assigning a
// fresh value (`h->lazy = LazyBufs{}`).

// One list set on the bound-pod table's rows: the list as its setter uploaded
// it (`ents` entries) and, after a commit, its second buffers.
struct KSIM_HIDDEN BoundList {
  DevPool bufs;
  size_t ents = 0;
};

// ksim_preempt_many's per-row slabs of one launch group, allocated at the
// first call that needs them (`rows` rows of PreemptNode[n] and of
// uint8_t[bound.n]), and ksim_preempt_many_dom's PreFilter states of one group
// of domain rows (`dom_rows` rows of int64[KSIM_MAX_USES][vmax] and of
// PreemptDomHead).  Sized by the bound table and the cluster: they go with the table.
struct KSIM_HIDDEN ManySlabs {
  DevPool bufs, dom_bufs;
  PreemptNode* res = nullptr;
  uint8_t* vflag = nullptr;
  int32_t rows = 0;
  int64_t* dom = nullptr;
  PreemptDomHead* heads = nullptr;
  int32_t dom_rows = 0;
};

// DefaultPreemption: the bound pods per node in importance order
// (ksim_set_bound_pods), the three lists set on their rows, and what
// ksim_preempt_commit keeps of the table.
struct KSIM_HIDDEN BoundPods {
  DevPool bufs;                         // the table, its second set and the scan's scratch
  DevPool nom_bufs;                     // ksim_preempt_nominated's group requests
  BoundList add, pdb, vol;              // ksim_set_bound_pod_adds, _pdbs, _volumes (vol: ksim_set_volume_limits drops it too)
  DevPreempt d{};
  int64_t* smin = nullptr;              // ksim_preempt_spread's per-use minima (k_preempt_spread_mins)
  const int32_t* voff = nullptr;        // [n + 1] CSR order: the rows' volume holdings (null: none set)
  const VolHold* vols = nullptr;
  std::vector<int32_t> index;           // CSR position -> bound-pod table index
  const int32_t* dindex = nullptr;      // its device copy (ksim_preempt_many)
  int32_t n = 0;                        // the caller's rows (ksim_set_bound_pods), evicted ones included
  int32_t maxrow = 0;                   // the most bound pods one node holds
  // ksim_preempt_commit.  Per caller's row: its node and requests as
  // ksim_set_bound_pods took them, and whether a commit evicted it since
  // (dead; 2 inside a call: named by it).  `live` rows are left, at the
  // table's positions [0, live).  A commit compacts the device's arrays and
  // leaves `index` as it was (index_stale): the setters compact it, and until
  // then a single dry run reads its victims' rows from dindex.  alt holds the
  // table's second buffer set and the scan's scratch (its *2 fields and pos /
  // dead / before / tile; null: not allocated), owned by bufs and, each
  // list's, by the list; every commit swaps the two sets.
  std::vector<int32_t> row_node;
  std::vector<int64_t> row_req;
  std::vector<uint8_t> dead;
  int32_t live = 0;
  bool index_stale = false;
  DevCommit alt{};
  ManySlabs many;
};

// Deferred-commit FAST batches (ksim_internal.h): the second snapshot buffer
// X[1] and state st[1], the ring of chain + pairs outputs, sized by dc.n
// (alloc_lazy; n: the node count they were allocated for, -1: none).
struct KSIM_HIDDEN LazyBufs {
  DevPool bufs;
  int32_t n = -1;
  DynCols x1{};
  DevState* st1 = nullptr;
  uint64_t *g = nullptr, *m = nullptr;             // [kLazySlots][kBatchPods]
  int32_t* e = nullptr;                            // [kLazySlots] prefix length, -1 = empty slot
  int32_t *ab = nullptr, *aw = nullptr;            // ADAPT: [kLazySlots][kBatchPods] broken flags, [..][2 B] windows
};

// Node-sharded ADAPT batch: this shard's bitmaps, the all-gathered ones and the
// global bitmap (adapt_shard_buffers: allocated at the first such run).
struct KSIM_HIDDEN AshBufs {
  DevPool bufs;
  uint64_t *send = nullptr, *recv = nullptr, *gmask = nullptr;
  int32_t world = 0, w = 0;
};

// Members are destroyed last to first: the stream and the events, which the
// buffers' frees may still need, come first.
struct ksim_handle {
  KSIM_HIDDEN ksim_handle() = default;   // (the library exports the C ABI, not this)
  int device = 0;
  HipStream stream;
  HipEvent ev0, ev1;
  std::string err;

  bool has_profile = false;
  ksim_profile prof{};
  BatchProg bp{};
  // device copies of prof / bp, read by the batch-path kernels: a captured
  // batch graph then survives a weight change (ksim_set_profile)
  ksim_profile* d_prof = nullptr;
  BatchProg* d_bp = nullptr;
  // what lives as long as the handle, at a fixed address: st, d_prof, d_bp
  // (ksim_create) and sweep_tab (alloc_sweep)
  DevPool life_bufs;
  std::vector<size_t> pod_buf_bytes;    // sizes of pod_bufs (ksim_load_pods reuses same-sized buffers)

  bool has_cluster = false;
  DevCluster dc{};
  DevPool cluster_bufs;
  std::vector<uint8_t> taint_effect;    // host copy (batchability analysis)
  std::vector<uint16_t> hard_taints;    // taint ids with effect NoSchedule/NoExecute on some node
  bool any_unschedulable = false;       // some node has spec.unschedulable
  bool alloc_narrow = false;            // every allocatable cpu / memory in [0, 2^46) (dyn_key_fast)

  // device copy of the uploaded dynamic columns (ksim_reset_cluster)
  struct {
    int64_t *req_cpu, *req_mem, *req_eph, *req_scalar, *nz_cpu, *nz_mem;
    int32_t *num_pods, *cnt;
    int64_t* nb_alloc;
  } init{};
  // node volume limits (ksim_set_volume_limits): limit, attached and the copy
  // of attached that ksim_reset_cluster restores
  DevPool vol_bufs;
  int32_t* vol_init = nullptr;
  std::vector<int32_t> col_nvals;       // host copy (pod validation)
  std::vector<uint8_t> col_unique;      // host copy of DevCluster.col_unique (kUseUniqueCol on upload)
  std::vector<uint8_t> col_total;       // per label column: every node carries the key

  DevScratch sc{};
  DevEvalOut eo{};
  DevPool scratch_bufs;

  DevState* st = nullptr;
  int32_t run_hdr[2] = {0, 0};

  // loaded pod queue (batch mode)
  DevPods dp{};
  DevPool pod_bufs;                     // the queue's arrays in ksim_load_pods' order, then d_chosen
  int32_t* d_chosen = nullptr;
  std::vector<uint8_t> batchable;       // per loaded pod
  std::vector<uint8_t> topo;            // per loaded pod: 0 no topology uses, 1 uses (k_topo_prefilter), 2 uses
                                        // read from persistent tables (kPlanPtab)
  std::vector<uint8_t> trivial;         // per loaded pod: kBatchStaticTrivial
  std::vector<uint8_t> noadd;           // per loaded pod: no count-class adds (deferred-commit batches)
  std::vector<uint8_t> noscalar;        // ... and no scalar requests (generic deferred-commit batches)
  // static classes (DevPods::stab, ensure_stab): per loaded pod its class or
  // -1 (d_sclass), each class's representative pod (d_srep); the table is
  // rebuilt after any change of pods, cluster or profile (stab_dirty)
  int32_t* d_sclass = nullptr;
  int32_t* d_srep = nullptr;
  int32_t stab_ncls = 0;
  bool stab_dirty = true, stab_ready = false;
  DevPool stab_bufs;
  size_t stab_bytes = 0;
  std::vector<int32_t> sclass;          // host copy of d_sclass
  std::vector<uint8_t> hard_small;      // per loaded pod: every hard spread key column has <= kFuseMinValues values
  std::vector<uint8_t> soft_le1;        // per loaded pod: at most one ScheduleAnyway spread constraint
  std::vector<int32_t> tlen;            // per loaded pod: topology batch run length from it (tbatch_runs)
  std::vector<int32_t> tlen_plain;      // ... without zone variants (replicated topology batches)
  std::vector<int64_t> xdom_len;        // per loaded pod: sharded cycle, packed domain words
  std::vector<int64_t> xreg_len;        // per loaded pod: sharded cycle, registration words (0: no soft spread)

  // compat-mode single pod
  DevGrow pod1_arena;                   // the single-pod uploads (upload_single)
  DevGrow nom_arena;                    // a nominated pod (ksim_fw_filter_nominated)
  // Reserve / Unreserve calls that arrive while a framework cycle sits between
  // its PreFilter and Score (the binding goroutine's Unreserve):
  // upstream's running cycle keeps its snapshot, so the engine applies them
  // once that cycle has scored (flush_deferred_binds), in call order
  struct DeferredBind {
    ksim_pod pod;
    std::vector<ksim_label_expr> ex;
    std::vector<ksim_term> tm;
    std::vector<ksim_topo_use> us;
    std::vector<ksim_class_add> ad;
    std::vector<int32_t> nn;
    int32_t node;
    int sign;
  };
  std::vector<DeferredBind> deferred_binds;
  // pinned, coherent host staging for the per-call uploads / results, and the
  // device's addresses of it (copy kernels read / write it directly)
  PinGrow pin{kPinMapped, 1 << 16, "hipHostMalloc (staging)"};
  // the last pod upload's copy out of the staging (upload_blob waits on it
  // instead of the whole stream); the pod last uploaded into pod1_arena (its
  // bytes and device address: a Reserve / Unreserve of the same pod binds
  // from there, no upload)
  // upload_blob's pinned staging ring: consecutive pod uploads (an informer's
  // pod deltas, another pod's Reserve, the next cycle's pod) do not wait for
  // each other's copies; a slot is reused once its copy has run (its event)
  struct PinSlot {
    PinGrow buf{kPinMapped, 1 << 14, "hipHostMalloc (upload ring)"};
    HipEvent ev;
    bool pending = false;
  };
  static constexpr int kPinRing = 4;
  PinSlot ring[kPinRing];
  int ring_next = 0;
  std::vector<char> pod1_blob;
  char* pod1_base = nullptr;
  // build_pod_blob's pieces and the framework-driven pass's blob, kept so the
  // per-cycle calls reuse their capacity
  std::vector<ksim_label_expr> bs_ex;
  std::vector<ksim_term> bs_tm;
  std::vector<ksim_topo_use> bs_us;
  std::vector<ksim_class_add> bs_ad;
  std::vector<int32_t> bs_nn;
  PodBlob fw_blob;
  // the framework-driven filter passes alternate two arenas, so the Reserve of
  // cycle i (binding from cycle i's arena) can wait, queued, and run inside
  // cycle i+1's upload launch (pend_bind); any other call launches it first
  DevGrow fw_arena[2];
  int fw_flip = 0;
  struct PendBind {
    bool on = false;
    DevPods P{};
    int32_t node = 0;
    int sign = 0;
  } pend_bind;
  int64_t pend_reuse = 0;                      // upload_blob found the queued Reserve's arena reused (flushed)
  PinGrow pout{kPinMapped, 1 << 16, "hipHostMalloc (results)"};
  BoundPods bound;                      // DefaultPreemption; dropped whole by ksim_set_bound_pods and ksim_set_cluster
  // ksim_preempt_many, with the handle: the call's preemptor records and row
  // table (one upload out of the pinned many_stage), the result buffer (pick
  // records, then the victims lists) and its pinned host copy many_host; every
  // call ends synchronized, so neither is in flight when the next call writes it.
  DevGrow many_arena, many_out;
  PinGrow many_stage{hipHostMallocDefault, 1 << 16, "hipHostMalloc (pinned buffer)"};
  PinGrow many_host{hipHostMallocDefault, 1 << 16, "hipHostMalloc (pinned buffer)"};
  size_t many_stage_bytes = 0;          // of the call in flight
  int64_t many_rows = 0, many_single = 0;   // rows answered by the batched / the single-pod launches (ksim_get_diag)
  int64_t many_dom_answered = 0;        // ksim_preempt_many_dom's domain rows, by the batched launches
  // extender round trip (ksim_eval_pod_filter -> ksim_eval_pod_finish)
  DevPods pod1{};
  bool ext_pending = false;
  uint8_t* ext_fail = nullptr;     // device [n]
  int64_t* ext_score = nullptr;    // device [n]
  // framework-driven compat cycle (ksim_fw_prefilter -> ksim_fw_score ->
  // ksim_fw_normalize): the pod in h->pod1, its filter pass on the host for
  // list validation, the scan-set size
  bool fw_pending = false, fw_scored = false, fw_dom_dirty = false, fw_topo = false;
  int32_t fw_ns = 0;
  std::vector<uint8_t> fw_fail;
  // ksim_fw_score's list and answers, host side: a NormalizeScore over that
  // list with the raw scores it returned is answered from here
  std::vector<int32_t> fw_list;
  std::vector<int64_t> fw_raw, fw_norm;         // [slot][list position]
  // host-answered Score (fw_host): ksim_fw_prefilter also copies every node's
  // raw scores, the weighted sum of the plugins without NormalizeScore and the
  // topology flags into pinned memory, and ksim_fw_score normalizes over the
  // framework's list on the host (no second device round trip) when no
  // PreScore of the pod depends on that list
  bool fw_host = false;
  int64_t fw_counts[4] = {0, 0, 0, 0};   // Score on the host / device, NormalizeScore cached / device
  std::vector<uint8_t> fw_seen;    // list validation (all zero between calls)
  std::vector<int64_t> fw_tot;
  PinGrow fwh{kPinMapped, 0, "hipHostMalloc (fw answers)"};   // [S][n] raw, [n] part
  uint32_t fw_tflags = 0;
  size_t fw_oraw = 0, fw_opart = 0;  // fwh offsets of the raw scores and the weighted part
  bool fw_raw32 = false;             // ... as int32 (the filter kernel's own copy) or int64 (a copy launch)
  int32_t* fw_nodes = nullptr;     // device [n]
  int64_t* fw_vals = nullptr;      // device [n]
  int64_t* fw_out = nullptr;       // device [n]

  // node sharding: this handle holds [shard_base, shard_base + n) of shard_total
  int32_t shard_base = 0, shard_total = 0;
  // replicated handle (ksim_set_eval_range): holds every node, evaluates
  // [eval_lo, eval_hi) in the P100 batch top-T and keeps its replica by
  // binding every placement: one exchange per batch (the records' all-gather)
  bool replicated = false;
  int32_t eval_lo = 0, eval_hi = 0;
  bool rep_primary = true;              // replicated: this replica counts the whole-run evaluations
  int32_t rank = 0, world = 1;
  ncclComm_t comm = nullptr;

  // every graph of this handle's own runs, by what it holds (ksim_engine.cpp
  // handle_graph captures them, drop_graphs_if destroys them)
  std::map<GraphKey, hipGraphExec_t> graphs;
  LazyBufs lazy;                        // deferred-commit batches (alloc_lazy)
  // run_lazy's progress words (host-mapped pinned; alloc_lazy reserves them
  // once, and the graphs hold their address): [0] the last state writer's
  // lazy_progress, [1] the batch counter the run started from
  PinGrow prog{kPinMapped, 0, "hipHostMalloc (progress word)"};
  // ksim_schedule_loaded leaves the zeroing of the call's counters to its first
  // run (run_range: run_lazy's begin launch takes it, every other run calls
  // reset_counters first)
  bool counters_pending = false;
  // deferred-commit runs since ksim_create (ksim_get_diag out[28..32]): host
  // synchronisations inside them, batches enqueued past the end of their run,
  // stretches ended by a flush and a state read instead of the progress word,
  // top-ups (batches enqueued after a run's first stretch, by the word or a
  // read), runs whose last flush had an odd ring index (the end launch copied
  // X[1] and st[1] back)
  int64_t feed_syncs = 0, feed_past_end = 0, feed_fallbacks = 0, feed_topups = 0, feed_odd_ends = 0;
  // request classes of the loaded queue (ksim_internal.h ReqTab): per loaded
  // pod its class (0xffff: none), the classes' requests, and the table's two
  // halves [2][rq_ncls][dc.n] with the ring's patch entries
  // [kLazySlots][rq_ncls][kBatchPods] behind them (ensure_rtab; a reallocation
  // drops the deferred-commit graphs of the runs that take the table)
  std::vector<uint16_t> rq_cls;
  uint16_t* d_rcls = nullptr;
  PodReq* d_rreq = nullptr;
  int32_t rq_ncls = 0;                             // > kReqMaxClasses: too many, no table
  DevPool rtab_bufs;
  size_t rtab_bytes = 0;
  int64_t rtab_runs = 0;                           // runs that took the table (ksim_get_diag out[27])
  AshBufs ash;                          // node-sharded ADAPT batches (adapt_shard_buffers)
  // packed policy sweep (ksim_sweep_loaded, run_sweep): the lanes' buffers as
  // one slab sized by (dc.n, lanes), the lane table [kLazySlots][kSweepMaxLanes]
  // (its address is all a sweep graph holds of them), the vectors' profile
  // copies, the lanes' placement rows
  struct SweepLaneBufs {
    DynCols x[2];
    uint64_t *g, *m;                             // [kLazySlots][kBatchPods]
    int32_t* e;                                  // [kLazySlots]
    uint64_t* topk;
    int32_t *topk_cnt, *topk_complete, *pinv;
    int64_t* pnorm;
  };
  DevPool sweep_slab;                            // one entry
  int32_t sweep_n = -1, sweep_lanes = 0;
  std::vector<SweepLaneBufs> sweep_lane;
  DevState* sweep_st = nullptr;                  // [sweep_lanes][2]
  SweepLane* sweep_tab = nullptr;                // in life_bufs
  DevGrow sweep_profs{0, "hipMalloc"}, sweep_rows{0, "hipMalloc"};
  // deferred-commit batches end at their first pair cut (KSIM_ONE_CUT=1 at the
  // last run's start): the setting the handle's deferred-commit graphs hold
  bool one_cut = false;
  int64_t graph_captures = 0;                  // graphs captured since ksim_create (ksim_get_diag)
  // shard-group graphs (group leader; ksim_engine.cpp group_graph): one graph
  // per GroupGraphKey, valid while the group is the handles of sg_sig, each at
  // the graph generation it had at capture; drop_group_graphs destroys them
  int64_t graph_gen = 0;                       // bumped whenever this handle's cycle graphs are dropped
  std::vector<std::pair<const ksim_handle*, int64_t>> sg_sig;
  std::map<GroupGraphKey, hipGraphExec_t> sg_graphs;
  bool sg_off = false;                         // group_graph failed once (e.g. a collective that cannot be captured)
  int64_t match_ns = 0;                        // device time of the last ksim_match_terms (HIP events)
};

#define HIPCHK(h, expr)                                    \
  do {                                                     \
    hipError_t _e = (expr);                                \
    if (_e != hipSuccess) return hip_fail((h), _e, #expr); \
  } while (0)

// Defined in ksim_engine.cpp, one copy each; hidden: the library exports the C ABI only.
namespace ksim_host __attribute__((visibility("hidden"))) {

int set_err(ksim_handle* h, int code, const std::string& msg);
int hip_fail(ksim_handle* h, hipError_t e, const char* what);
hipError_t hcopy(ksim_handle* h, void* dst, const void* src, size_t bytes, hipMemcpyKind kind);
void drop_graphs(ksim_handle* h);
void drop_loaded_pods(ksim_handle* h);
bool is_sharded(const ksim_handle* h);
int validate_pod(ksim_handle* h, const ksim_pod_set* ps, int32_t i);
int flush_pend_bind(ksim_handle* h);
int flush_idle(ksim_handle* h);
int ensure_ready(ksim_handle* h, bool fw = false, bool keep_pend = false);
LaunchArgs make_args(ksim_handle* h, const DevPods& P, int32_t* chosen);
int set_run(ksim_handle* h, int32_t first, int32_t end);
int upload_single(ksim_handle* h, const ksim_pod_set* ps, int32_t pod_index, DevPods& P, DevGrow& arena);
int upload_single(ksim_handle* h, const ksim_pod_set* ps, int32_t pod_index, DevPods& P);
// Pods idx[0 .. n) of ps, each as upload_single would upload it, packed into
// h->many_stage with `extra` more bytes behind them (64-byte aligned), and
// h->many_arena grown to hold it all.  Ps[i]: pod i's device set; extra_host /
// extra_dev: the extra bytes in the staging and where they land.  Nothing is
// copied yet: the caller fills the extra bytes, then upload_many_commit
// enqueues the one copy.
int upload_many(ksim_handle* h, const ksim_pod_set* ps, const int32_t* idx, int32_t n, size_t extra,
                std::vector<DevPods>& Ps, char** extra_host, char** extra_dev);
int upload_many_commit(ksim_handle* h);
}  // namespace ksim_host
