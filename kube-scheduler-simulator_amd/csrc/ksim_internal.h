// ksim_internal.h — launcher interface between the host runtime
// (ksim_engine.cpp) and the kernels (ksim_kernels.hip).
#pragma once

#include "ksim_device.h"

namespace ksim {

// A/B forms of the same runs, chosen at compile time (csrc/Makefile "ab":
// libksim_engine_ab.so, every alternative form on; tests/test_gpu_ab_switches.py
// runs it against the oracle).  The product library has none of them.
// KSIM_AB_FORMS is a bitmask of the alternative forms (csrc/Makefile "ab":
// 255, every one on; "abforms": one form each, checked against the product's
// other forms):
constexpr unsigned kAbStab = 1;      // per-node static plugins (no static-class table)
constexpr unsigned kAbLazy = 2;      // three-launch batches (commit as its own launch)
constexpr unsigned kAbAdaptNorm = 4; // ADAPT normalized-score pods on the per-pod path
constexpr unsigned kAbTbatch = 8;    // topology pods on the per-pod path
constexpr unsigned kAbShardGraph = 16;   // eager shard cycles (no shard-group graphs)
constexpr unsigned kAbPtab = 32;     // per-cycle PreFilter domain sums (no persistent tables)
constexpr unsigned kAbTbVar = 64;    // topology batches end at a zone-keyed class conflict (no zone variants)
constexpr unsigned kAbReqTab = 128;  // KEEP/DEF deferred-commit batches key every pod x node pair (no request-class table)
#ifdef KSIM_AB_FORMS
constexpr unsigned kAbMask = KSIM_AB_FORMS;
#else
constexpr unsigned kAbMask = 0;
#endif
constexpr bool ab(unsigned form) { return (kAbMask & form) != 0; }


// Batch path geometry.
// Compile-time overridable for A/B builds (-DKSIM_BATCH_PODS=512 -DKSIM_TOP_T=16).
#ifndef KSIM_BATCH_PODS
#define KSIM_BATCH_PODS 256
#endif
#ifndef KSIM_TOP_T
#define KSIM_TOP_T 8
#endif
constexpr int kBatchPods = KSIM_BATCH_PODS;   // B: pods per speculative batch
constexpr int kTopT = KSIM_TOP_T;             // T: candidate keys kept per pod
constexpr int kMaxListRecords = 4;            // list records per pod (ksim_batch.hip kNsSlices)
static_assert(kBatchPods % 64 == 0 && kBatchPods <= 1024 && kTopT <= 64, "batch geometry");
constexpr int kTopThreads = 1024;  // threads per pod of the batch top
constexpr int kTileCand = 4;       // best keys each lane of the batch top keeps per pod
constexpr int kKeepPerLane = 8;    // KEEP evaluation forms: keys a lane holds in registers (ksim_batch.hip)
constexpr int kXRec = kTopT + 1;   // sharded exchange record per pod: T keys + (count | complete << 32)
#ifndef KSIM_MAX_SHARDS
#define KSIM_MAX_SHARDS 8
#endif
constexpr int kMaxShards = KSIM_MAX_SHARDS;   // shards of one simulation (one per GPU of a node)
constexpr int kGmergeSlots = (kTopT * kMaxShards + 63) / 64;   // list entries per lane in k_batch_gmerge
static_assert(kGmergeSlots <= 2, "gmerge geometry");

// In-process shard group (one device): the pmax arrays of up to kMaxShards handles.
struct GroupPtrs {
  uint64_t* p[kMaxShards];
  int32_t n;
};

struct LaunchArgs {
  DevCluster c;
  DevPods P;
  ksim_profile prof;
  BatchProg bp;
  DevState* st;
  DevScratch s;
  DevEvalOut o;
  int32_t* chosen;   // [n_pods] device, may be null
  const ksim_profile* dprof = nullptr;   // device copies of prof / bp (the batch kernels read these)
  const BatchProg* dbp = nullptr;
  bool fast = false; // batch runs: every pod trivial and cpu/memory scoring (k_batch_top<true>)
  bool stab = false; // ... or (with fast) every pod in a static class (DevPods::stab; the STAB kernels)
  bool fuse_min = false;  // per-pod topology runs: every hard spread key has <= 256 values
  bool fuse_ext = false;  // per-pod runs: every pod has <= 1 ScheduleAnyway spread constraint (K = N: no k_extrema)
  bool ptab = false;      // per-pod topology runs: every pod carries kPlanPtab (no k_topo_prefilter)
};

constexpr int kKernelsPerCycle = 7;
constexpr int kFuseMinValues = 256;   // k_filter_score computes the PTS critical paths itself up to this many values
extern const char* const kKernelNames[kKernelsPerCycle];
constexpr int kKernelsPerBatch = 3;
extern const char* const kBatchKernelNames[kKernelsPerBatch];
constexpr int kKernelsPerAdapt = 5;
extern const char* const kAdaptKernelNames[kKernelsPerAdapt];
// Topology batch path (ksim_tbatch.hip): at most kTbPods pods per batch (the
// host's runs, bflags >> kTlenShift), clusters of at most kTbMaxBlocks node
// blocks of 256.  A run may cross a class an earlier pod of it adds when every
// use that reads it is node-local (tbatch_conflict_ok; the pairs step re-keys
// the guessed node; the run's first pod carries kPodTbCross).
constexpr int kTbPods = 32;
constexpr int kTbMaxBlocks = 64;
constexpr int kKernelsPerTbatch = 5;
extern const char* const kTbatchKernelNames[kKernelsPerTbatch];
uint32_t launch_tbatch(const LaunchArgs& a, hipStream_t stream, hipEvent_t* evs = nullptr);
// Replicated topology batches (every replica holds the whole snapshot and
// evaluates its node range [c.eval_lo, c.eval_hi)); the caller exchanges
// between the phases:
//   launch_tb_rep_filter   filter + raw scores + per-pod counters / extrema
//                          (all-gather s.tb_win -> s.tb_xrecv [world][kTbPods])
//   launch_tb_rep_select   merged counters, totals + keys, holders, the
//                          replica's per-pod top-T record
//                          (all-gather s.xsend -> s.xrecv [world][kTbPods][kTbXRec])
//   launch_tb_rep_pairs    global top-T, chain, pair keys of the guesses this
//                          replica evaluated (all-reduce max s.tb_pp)
//   launch_tb_rep_commit   commit on every replica (every bind, every class add)
constexpr int kTbXRec = kTopT + 1 + KSIM_MAX_SCORE;   // T keys, count, holder counts (2 x int32 per slot)
void launch_tb_rep_filter(const LaunchArgs& a, hipStream_t stream);
void launch_tb_rep_select(const LaunchArgs& a, int32_t world, hipStream_t stream);
void launch_tb_rep_pairs(const LaunchArgs& a, int32_t world, hipStream_t stream);
void launch_tb_rep_commit(const LaunchArgs& a, hipStream_t stream);

// One scheduling cycle for the pod at st->cursor (no-op once cursor >= end).
// evs (nullable, kKernelsPerCycle + 1 events) are recorded around each kernel.
// topo: the pod may carry PodTopologySpread / InterPodAffinity uses (adds the
// two topology kernels; they exit at once for a pod without uses).
// Returns the kernel slots it launched (bit k: kernel k of the cycle), so a
// timing run counts only those.
uint32_t launch_cycle(const LaunchArgs& a, hipStream_t stream, bool compat, bool topo, hipEvent_t* evs = nullptr);
// One speculative batch of up to kBatchPods pods from st->cursor (>= 1 committed).
// Returns the mask of kernel slots launched (bit k: kBatchKernelNames[k]).
unsigned long long* adapt_dbg_buffer();  // KSIM_ADAPT_DBG builds: why ADAPT batches end short (else null)
unsigned long long* cp_clock_buffer();   // KSIM_CP_CLOCKS builds: chain + pairs phase clocks (else null)
uint32_t launch_batch(const LaunchArgs& a, hipStream_t stream, hipEvent_t* evs = nullptr);
// The same under ADAPT (K < N): windows by relaxation, see ksim_adapt.hip.
uint32_t launch_batch_adapt(const LaunchArgs& a, hipStream_t stream, hipEvent_t* evs = nullptr);

// ---- deferred-commit FAST batches (ksim_batch.hip k_batch_top_commit) ---------
// Batch i's commit runs inside batch i+1's evaluation launch: two launches per
// batch instead of three.  The dynamic node columns are double-buffered: batch
// i evaluates the snapshot X[p ^ 1] (p = i & 1) that batch i-1 evaluated, plus
// batch i-1's binds as an overlay, and writes S_i into X[p] for the nodes batch
// i-1 or i-2 bound (X[p] held S_{i-2}); its chain + pairs then read X[p].  The
// chain + pairs outputs (guess keys, pair maxima, prefix length) live in a
// ring of kLazySlots slots, slot i & 3.  X[0] and st[0] are the handle's own.
constexpr int kLazySlots = 4;
constexpr int kLazyMaxNodes = 1 << 17;   // the overlay's LDS node bitmap (16 KB)
constexpr int kLazyHashBits = 10;        // overlay hash: node -> entry, >= 4 x kBatchPods slots
struct DynCols {
  int64_t *req_cpu, *req_mem, *req_eph, *nz_cpu, *nz_mem;
  int32_t* num_pods;
};
// Request classes (ReqTab): the pods of a loaded queue that share their five
// request fields share a class, and T[2][C][N] holds each class's verdict and
// scores on each node (req_entry), double-buffered with X: batch i reads
// T[p ^ 1] (S_{i-1}; the nodes batch i-1 bound patched from P, below) and
// writes S_i's entries into T[p] for the nodes batches i-1 and i-2 guessed,
// exactly where it writes X[p].  k_req_table fills both halves from X at the
// start of a run.  n_cls = 0: no table (every other launch form).
// The patch entries P[kLazySlots][C][kBatchPods] ride the ring: batch i's
// pairs launch, whose thread k holds S_i[node(g_k)] + pod k for its pair key,
// writes every class's entry of that row into slot i & 3 (block B - 1 - c keys
// class c for every k of the chain: one 512-byte row per class), and batch
// i + 1's evaluation launch reads its class's row of that slot, entry t under
// t < i* <= chain_end only, so a stale slot or a stale tail is never selected.
// Only the node that takes two pods at a cut is keyed in the evaluation launch.
// The pod records H[2][2 * kBatchPods] ride the batch parity like st[] / X[]:
// batch i's evaluation launch, once it knows where batch i starts (base),
// writes the records of pods base + [0, 2 * kBatchPods) into H[p] (block b its
// own pod base + b and pod base + kBatchPods + b), and batch i + 1's reads its
// 2 * kBatchPods + 1 records (batch i's requests, its own candidates) from
// there, at addresses that do not depend on the state's cursor.  A flush
// writes them too; reqtab_begin fills H[1] at a run's start.
constexpr int kReqMaxClasses = 256;
struct alignas(16) PodRec {
  PodReq req;                                      // zero past the run's end
  uint16_t cls, valid;                             // request class; 1: the pod is before the run's end
  uint32_t _pad;
};
static_assert(sizeof(PodRec) == 48, "pod record: three 16-byte words");
constexpr uint16_t kNoClass = 0xffff;              // s_cls of a record past the run's end
struct ReqTab {
  const uint16_t* t_in = nullptr;                  // T[p ^ 1], [n_cls][n]
  uint16_t* t_out = nullptr;                       // T[p]
  const PodReq* rreq = nullptr;                    // [n_cls] the classes' requests
  const uint16_t* rcls = nullptr;                  // [n_pods] class of each loaded pod
  const uint16_t* p_in = nullptr;                  // P[(i - 1) & 3], [n_cls][kBatchPods]: batch i-1's patch entries
  uint16_t* p_out = nullptr;                       // P[i & 3]: batch i's, written by its pairs launch
  const PodRec* h_in = nullptr;                    // H[p ^ 1]: the records batch i-1's evaluation launch wrote
  PodRec* h_out = nullptr;                         // H[p]: batch i's, for batch i+1
  int32_t n_cls = 0, _pad = 0;
};
struct LazyStep {
  DynCols w;                                       // X[p]: receives S_i
  const DevState* st_in;                           // st[p ^ 1]: the state batch i-1 started from
  DevState* st_out;                                // st[p]: after batch i-1's commit
  const uint64_t* g1; const uint64_t* m1; const int32_t* e1;   // batch i-1's slot: guesses, pair maxima, prefix
  const uint64_t* g2; const int32_t* e2;                       // batch i-2's slot: guesses, prefix
  int32_t* e_self;                                 // batch i's slot (a flush marks it empty: -1)
  // run_lazy's progress word (host-mapped, null: none): the state writer
  // stores lazy_progress(cursor, batches) of the state it wrote
  unsigned long long* prog = nullptr;
  // 1: batch i-1 ends at its first pair cut (KSIM_ONE_CUT=1, read per run);
  // 0: it goes on through the second stretch (ksim_batch.hip)
  int32_t one_cut = 0, _pad = 0;
};
// The progress word: the cursor after the launch's commit above the handle's
// batch counter (DevState::batches, which counts committed batches).
__host__ __device__ inline unsigned long long lazy_progress(int32_t cursor, int32_t batches) {
  return ((unsigned long long)(uint32_t)cursor << 32) | (uint32_t)batches;
}
// How many more batches run_lazy may enqueue without one starting past the
// end: `left` pods remain after the last commit the host has seen and
// `pending` enqueued batches start at or after it; a batch commits at most
// kBatchPods pods, so ceil(left / kBatchPods) batches never pass the end.
constexpr int32_t lazy_more_batches(int32_t left, int32_t pending, int32_t batch_pods) {
  // ((left - 1) / B + 1: no overflow near INT32_MAX)
  return left <= 0 ? 0 : ((left - 1) / batch_pods + 1 > pending ? (left - 1) / batch_pods + 1 - pending : 0);
}
struct LazyBatch {
  LaunchArgs a;        // a.c: static columns + X[p ^ 1]
  DevCluster cw;       // static columns + X[p]
  LazyStep step;
  ReqTab rt;           // the request-class table halves of the batch (run_lazy's runs that take it)
  DevState* st;        // st[p]
  uint64_t* gkey;      // batch i's slot
  uint64_t* pmax;
  int32_t* cend;
  // ADAPT: batch i-1's broken-window flags and windows, batch i's slot of them
  const int32_t* b1;
  const int32_t* w1;
  int32_t* abroken;
  int32_t* awin;
};
// Packed policy sweep (ksim_sweep_loaded; ksim_batch.hip k_sweep_*): the two
// launches of a deferred-commit batch with gridDim.y lanes, each lane a run of
// its own (its two dynamic-column sets, states, ring, lists, placements row)
// under its own profile copy, over the shared static columns and pod queue.
// One record per (batch index & 3, lane): what LazyBatch holds for the batch.
constexpr int kSweepMaxLanes = 64;
struct SweepLane {
  DynCols x_in;                                    // X[p ^ 1]
  LazyStep step;                                   // step.w: X[p]; st_out: st[p]; e_self: batch i's slot
  uint64_t* gkey;                                  // batch i's slot
  uint64_t* pmax;
  uint64_t* topk;
  int32_t* topk_cnt;
  int32_t* topk_complete;
  int64_t* pnorm;
  int32_t* pinv;
  int32_t* chosen;                                 // the lane's placements row, by loaded pod index
  const ksim_profile* prof;                        // the lane's vector
  const BatchProg* bp;
};
void launch_sweep_batch(const DevCluster& c, const DevPods& P, const SweepLane* tab, int32_t lanes, bool def,
                        hipStream_t stream);
void launch_sweep_flush(const DevCluster& c, const DevPods& P, const SweepLane* tab, int32_t lanes, hipStream_t stream);
constexpr int kKernelsPerLazy = 2;
extern const char* const kLazyKernelNames[kKernelsPerLazy];
// ADAPT (ksim_adapt.hip): k_adapt_mask_commit (commit of i-1, the S_i bitmaps
// of i, every row written to X[p]), the window scan when not fused into the
// top, the top, the chain + pairs.  X[p] is written whole, so only batch i-1's
// slot is read.
constexpr int kKernelsPerLazyAdapt = 4;
extern const char* const kLazyAdaptKernelNames[kKernelsPerLazyAdapt];
uint32_t launch_batch_adapt_lazy(const LazyBatch& z, hipStream_t stream, hipEvent_t* evs = nullptr);
void launch_adapt_lazy_flush(const LazyBatch& z, hipStream_t stream);
// batch i: k_batch_top_commit (commit of i-1, evaluation of i), then the
// chain + pairs of i.  A flush is the first launch alone with no evaluation:
// it commits batch i-1 and leaves slot i empty.
// DevPods::stab rows of classes [0, n_cls) (ksim_batch.hip k_static_table)
void launch_static_table(const LaunchArgs& a, const int32_t* rep, int32_t n_cls, uint64_t* stab, hipStream_t stream);
uint32_t launch_batch_lazy(const LazyBatch& z, hipStream_t stream, hipEvent_t* evs = nullptr);
// both halves of the request-class table from the snapshot a.c (k_req_table)
void launch_req_table(const LaunchArgs& a, const ReqTab& rt, uint16_t* t0, uint16_t* t1, hipStream_t stream);
// the pod records of pods first + [0, 2 * kBatchPods) of a run that ends at `end` (k_req_records)
void launch_req_records(const LaunchArgs& a, const ReqTab& rt, int32_t first, int32_t end, PodRec* out,
                        hipStream_t stream);
void launch_lazy_flush(const LazyBatch& z, hipStream_t stream);
// the evaluation-launch instantiations launched so far (ksim_get_diag out[25])
uint64_t batch_variant_reach();
void launch_lazy_top(const LazyBatch& z, hipStream_t stream);   // the first launch alone (ksim_time_eval)
// replicated handles: the first launch with the replica's record (xsend), then,
// after the records' all-gather into a.s.xrecv, the global merge + chain + pairs
void launch_lazy_top_rep(const LazyBatch& z, uint64_t* xsend, hipStream_t stream);
void launch_lazy_chain_rep(const LazyBatch& z, int32_t world, hipStream_t stream);
// Compat cycle around the host's extender round trip (ksim_eval_pod_filter / _finish):
// the filter pass + window, then (a.s.ext_fail / ext_score set) the rest.
void launch_cycle_filter(const LaunchArgs& a, hipStream_t stream, bool topo);
void launch_cycle_finish(const LaunchArgs& a, hipStream_t stream);
// Framework-driven compat cycle (ksim_fw_*): Filter of every scanned node; then
// PreScore / Score / NormalizeScore over the framework's list (a.s.ext_fail =
// 1 for unlisted nodes), no bind; NormalizeScore of one slot over an explicit list.
void launch_fw_filter(const LaunchArgs& a, hipStream_t stream, bool topo);
void launch_fw_score(const LaunchArgs& a, hipStream_t stream);
constexpr int kCopyPieces = 8;
struct CopyList {
  const uint8_t* src[kCopyPieces];
  uint8_t* dst[kCopyPieces];
  uint32_t n[kCopyPieces];
  // optional (bst non-null): a framework-driven filter pass's start in the same
  // launch (launch_fw_begin's work, by block (0, 0))
  DevState* bst;
  WinState* bwin;
  int32_t bfirst, bend;
  // optional (anode >= 0): a queued Reserve / Unreserve (assume_pod of pod 0 of
  // aP on node anode, sign asign) in the same launch, by block (0, 0)
  int32_t anode, asign;
  DevCluster ac;
  DevPods aP;
};
void launch_copy_list(const CopyList& l, int count, hipStream_t stream);
// ksim_update_node_rows: packed static-column records of n rows (words int64 each)
void launch_node_rows(const DevCluster& c, const int64_t* rec, int32_t n, int32_t words, hipStream_t stream);
void launch_fw_gather(const DevEvalOut& o, const int32_t* nodes, int32_t n, int32_t N, int32_t S, int64_t* comp,
                      const WinState* win, void* win_out, hipStream_t stream);
void launch_fw_begin(DevState* st, WinState* win, int32_t first, int32_t end, hipStream_t stream);
void launch_fw_normalize(const LaunchArgs& a, int32_t slot, const int32_t* nodes, const int64_t* vals, int32_t n,
                         int64_t* out, hipStream_t stream);
// DefaultPreemption dry run (ksim_preempt.hip): the bound pods per node in
// importance order (CSR over nodes), per-node results, the pick.
constexpr uint8_t kPreemptViolating = 2;                     // DevPreempt.vflag bit 1 (bit 0: victim)
struct PreemptNode {
  // potential node; candidate (bit 0) and, above it, nviol: the victims that violate a PDB; victims;
  // victims[0]'s priority
  int32_t potential, cand, nv, high;
  int64_t sum, early;                  // sum of (priority + 2^31), earliest start of the highest-priority victims
  __host__ __device__ int32_t nviol() const { return cand >> 1; }
};
struct DevPreempt {
  const int32_t* off;                  // [n + 1]
  const int32_t* prio;                 // [n_bound] CSR order
  const int64_t* start;                // [n_bound]
  const int64_t* req;                  // [n_bound][KSIM_PREEMPT_REQ]
  uint8_t* vflag;                      // [n_bound] bit 0: victim of its node's dry run, bit 1: violates a PDB there
  PreemptNode* res;                    // [n]
  int32_t* pick;                       // [5] nominated, victims, potential, candidates kept, the node's PDB violations
  int32_t* nslot;                      // [n] nominated group of the node, -1: none
  const int64_t* nreq;                 // [groups][KSIM_PREEMPT_REQ + 1] requests, pod count
  // class contributions (ksim_set_bound_pod_adds; read only for a preemptor with NodePorts or
  // required pod (anti-)affinity uses)
  const int32_t* aoff;                 // [n_bound + 1] CSR order: adds[aoff[j] .. aoff[j + 1]) of bound pod j
  const ksim_class_add* adds;          // the bound pods' count-class contributions
  const int32_t* goff;                 // [groups + 1] the same per nominated group
  const ksim_class_add* gadds;
  int64_t* afftot;                     // [KSIM_MAX_USES] cluster-wide totals of the preemptor's required-affinity uses
  // PodDisruptionBudgets (ksim_set_bound_pod_pdbs; null: none, the dry run takes the forms without them)
  const int32_t* poff;                 // [n_bound + 1] CSR order: pids[poff[j] .. poff[j + 1]) the budgets bound pod j matches
  const int32_t* pids;
  const int32_t* pallowed;             // [n_pdbs] status.disruptionsAllowed
};
// One counted-volume holding of a bound pod or of a nominated pod: the device
// form of a KSIM_USE_VOLUME use (ksim_set_bound_pod_volumes).
struct VolHold {
  int32_t cls;                         // the shared volume's count class, -1: `arg` volumes nobody else holds
  int32_t fam;                         // family index < vol_nf
  int32_t arg;
};
// What the dry run's volume side reads (a preemptor with KSIM_USE_VOLUME uses:
// the volume form and the full form; the other forms' kernels do not take it).
// Only what the profile's limit plugins read is named: a family whose plugin
// the filter list lacks is in none of the masks.
struct PreemptVol {
  const int32_t* voff;                 // [n_bound + 1] CSR order: vols[voff[j] .. voff[j + 1]) of bound pod j
  const VolHold* vols;
  const int32_t* gvoff;                // [groups + 1] the same per nominated group (null without groups)
  const VolHold* gvols;
  uint32_t uses;                       // the preemptor's volume uses (bit i = use i)
  uint32_t fams;                       // the families they name (bit f)
  uint32_t csi;                        // those under NodeVolumeLimits' rule (new > 0)
  uint32_t at;                         // byte k: the profile position of plugin KSIM_PL_EBS_LIMITS + k, 0xff: absent
};
// Which uses of the preemptor one dry run reads, and where their filters stand.
struct PreemptPlan {
  int32_t fit, port, ipa, pts;         // NodeResourcesFit's, NodePorts', InterPodAffinity's, PodTopologySpread's places (-1: absent)
  int32_t prio;                        // the preemptor's priority
  // Its NodePorts, required-affinity, required-anti-affinity, existing-anti-affinity and DoNotSchedule
  // spread uses (bit i = use i).  A use whose filter the profile lacks is in none of them.
  uint32_t ports, aff, anti, exist, hard;
  int64_t* smin;                       // [KSIM_MAX_USES][3] device words for k_preempt_spread_mins' minima
  PreemptVol vol;                      // voff: null for a preemptor without volume uses
  bool vb, vz;                         // it has volume groups and VolumeBinding / VolumeZone is in the filter list
  // the node kernel reads the status pass's domain tables (a form with a row side)
  bool reads_domains() const { return (aff | anti | exist | hard) != 0; }
};
// One dry run over the statuses in s.fail (reads_domains(): and the status pass's domain tables
// in s.dom): the node kernel of the plan's form (ksim_preempt.hip), the static veto (vb / vz), the pick.
void launch_preempt(const LaunchArgs& a, const DevPreempt& pre, const PreemptPlan& plan, hipStream_t stream);

// The batched dry run (ksim_preempt_many): one launch group answers up to
// kPreemptManyRows preemptors whose plans read no domain table, thread =
// (node, row).  Every row owns what its dry run writes: a slab of per-node
// results and one of victim flags, so rows of different priority never share a
// mutable word.  One record per row, read at a block-uniform address.
constexpr int kPreemptManyRows = 64;                         // KSIM_PREEMPT_MANY_ROWS
constexpr size_t kPreemptManySlabBytes = (size_t)256 << 20;  // the slabs of one group stay under this
constexpr int kPickWords = 8;                                // int32 words per pick record (five used)
struct PreemptRow {
  DevPods P;                           // the preemptor as pod 0 of a set of its own
  PreemptVol vm;                       // voff: null for a row without volume uses
  PreemptNode* res;                    // [n] the row's slab
  uint8_t* vflag;                      // [n_bound] likewise
  int32_t* victims;                    // [cap] the nominated node's victims, caller indices
  int32_t cap;
  int32_t prio;
  uint32_t ports;                      // PreemptPlan::ports
  int32_t vb, vz;                      // PreemptPlan::vb / vz
};
// Rows per launch group for a cluster of n nodes and a table of n_bound rows
// (ksim_preempt_many_rows): rows x (sizeof(PreemptNode) n + n_bound) <= kPreemptManySlabBytes.
constexpr int32_t preempt_many_rows(int64_t n, int64_t n_bound) {
  const int64_t per = (int64_t)sizeof(PreemptNode) * (n > 0 ? n : 0) + (n_bound > 0 ? n_bound : 0);
  const int64_t fit = per > 0 ? (int64_t)kPreemptManySlabBytes / per : kPreemptManyRows;
  return (int32_t)(fit < 1 ? 1 : fit > kPreemptManyRows ? kPreemptManyRows : fit);
}
struct PreemptMany {
  const PreemptRow* rows;              // the group's rows (device)
  int32_t n_rows;
  bool volume;                         // the group's form: VolumeForm, else FreeForm / PortsForm
  PreemptNode* res;                    // [n_rows][n] the group's result slabs (row r's record names res + r n)
  int32_t* pick;                       // [n_rows][kPickWords] the group's pick records
  const int32_t* index;                // [n_bound] CSR position -> bound-pod table index (device)
  uint64_t rank_lo, rank_hi;           // BatchProg's filter positions (FilterPlan)
};
// One group: the node kernel of the group's form (status step, victims, static
// veto), the pick of every row, the victims lists.  pre: the table's shared,
// read-only arrays (res / vflag / pick / nslot of it are not read).
void launch_preempt_many(const LaunchArgs& a, const DevPreempt& pre, const PreemptPlan& common, const PreemptMany& g,
                         hipStream_t stream);

// ksim_preempt_many_dom: a row whose plan reads domain tables gets a PreFilter
// state of its own, the per-handle words of a single dry run once per row: the
// domain tables (dom, load_topo_row's indexing: [KSIM_MAX_USES][vmax]) and the
// small words beside them.  What a row reads of both is zero when its group starts.
struct PreemptDomHead {
  int64_t min_match[KSIM_MAX_USES];    // DevScratch.min_match: per DoNotSchedule use, the minimum over the present pairs
  int64_t smin[KSIM_MAX_USES][3];      // PreemptPlan.smin: {min1, the arg-min's value id, min2}
  int64_t afftot[KSIM_MAX_USES];       // DevPreempt.afftot
  uint32_t topo_flags;                 // DevState.topo_flags (kTopoAffinityNonEmpty alone: nothing scores)
  uint32_t _pad;
};
// Row k's record beside PreemptRow k (the same blockIdx.y).
struct PreemptDomRow {
  int64_t* dom;                        // [KSIM_MAX_USES][vmax] the row's tables
  PreemptDomHead* head;
  uint32_t aff, anti, exist, hard;     // PreemptPlan's masks of the row
};
// Rows per launch group of domain rows (ksim_preempt_many_dom_rows): the
// results, the flags and the tables of a group stay under kPreemptManySlabBytes.
constexpr int32_t preempt_many_dom_rows(int64_t n, int64_t n_bound, int64_t n_values) {
  const int64_t per = (int64_t)sizeof(PreemptNode) * (n > 0 ? n : 0) + (n_bound > 0 ? n_bound : 0) +
                      8 * (int64_t)KSIM_MAX_USES * (n_values > 0 ? n_values : 0);
  const int64_t fit = per > 0 ? (int64_t)kPreemptManySlabBytes / per : kPreemptManyRows;
  return (int32_t)(fit < 1 ? 1 : fit > kPreemptManyRows ? kPreemptManyRows : fit);
}
struct PreemptManyDom {
  const PreemptDomRow* drows;          // the group's rows (device), beside PreemptMany.rows
  bool full;                           // the group's form: FullForm, else SpreadForm (hard may be empty)
  bool spread;                         // some row of the group has a DoNotSchedule use (k_preempt_many_mins runs)
};
// One group of domain rows: what the rows read of their tables and heads zeroed
// (k_preempt_many_zero), every row's PreFilter pass (k_preempt_many_dom) and
// minima (k_preempt_many_mins), then the node kernel of the group's row form,
// the picks and the victims lists.
void launch_preempt_many_dom(const LaunchArgs& a, const DevPreempt& pre, const PreemptPlan& common,
                             const PreemptMany& g, const PreemptManyDom& d, hipStream_t stream);

// ksim_preempt_commit (ksim_preempt.hip "committed preemption"): the victims
// leave the snapshot and the bound table's rows are compacted in place, into
// the table's second buffer set.  A scan tile is kCommitTile rows: one block of
// kCommitThreads threads, kCommitTile / kCommitThreads consecutive rows each.
constexpr int kCommitThreads = 256;
constexpr int kCommitTile = 1024;                            // KSIM_COMMIT_TILE (ksim/preemption.py)
struct CommitRec {                     // one victim
  DevPods P;                           // its pod record as pod 0 of a set of its own
  int32_t row, node;                   // the caller's row number, the row's node
};
struct CommitSum {                     // what the scan carries per row: dead rows, surviving list entries
  int32_t dead, adds, pids, vols;
};
struct DevCommit {
  int32_t n, n_nodes;                  // rows before the commit, nodes
  // the table as it is (a list's offsets null: not set) ...
  const int32_t *off, *prio, *index;
  const int64_t *start, *req;
  const int32_t* aoff;
  const ksim_class_add* adds;
  const int32_t *poff, *pids;
  const int32_t* voff;
  const VolHold* vols;
  // ... and the second buffer set the survivors go to
  int32_t *off2, *prio2, *index2;
  int64_t *start2, *req2;
  int32_t* aoff2;
  ksim_class_add* adds2;
  int32_t *poff2, *pids2;
  int32_t* voff2;
  VolHold* vols2;
  // scratch, kept with the table
  int32_t* pos;                        // [rows of ksim_set_bound_pods] caller's row -> position
  uint8_t* dead;                       // [n + 1] the position leaves (position n: the end, never dead)
  int32_t* before;                     // [n + 1] dead rows before the position
  CommitSum* tile;                     // [tiles] each tile's sums, then (k_commit_carry) the sums before it
};
// Positions 0 .. n are scanned (position n carries the lists' end offsets).
constexpr int32_t commit_tiles(int32_t n) { return n / kCommitTile + 1; }
// The launches of one commit: victims recs[0 .. n_victims) evicted, the table compacted.
void launch_preempt_commit(const DevCluster& c, const DevCommit& m, const CommitRec* recs, int32_t n_victims,
                           hipStream_t stream);

// The evaluation kernels alone (ksim_time_eval).
void launch_batch_eval_only(const LaunchArgs& a, hipStream_t stream);
// topo: the pod carries uses; the PreFilter pass of its cycle runs first (the
// caller re-zeroes the domain tables and the topology flags afterwards)
void launch_filter_only(const LaunchArgs& a, hipStream_t stream, bool topo = false);
// Sharded batch (node shards; the caller exchanges between the phases):
//   launch_shard_eval    batch top; writes this shard's records to s.xsend
//   (all-gather s.xsend -> s.xrecv [world][kBatchPods][kXRec])
//   launch_shard_chain   global merge + chain + pair keys of owned guesses -> s.pmax
//   (all-reduce max s.pmax)
//   launch_shard_commit  validate + commit (owner shard binds)
void launch_shard_eval(const LaunchArgs& a, hipStream_t stream);
// records all-gathered in s.xrecv ([world][kBatchPods][kXRec]) -> per-pod global top-T
void k_batch_gmerge_launch(const LaunchArgs& a, int32_t world, hipStream_t stream);
// node-sharded ADAPT batch (ksim_adapt.hip): shard bitmaps of W words per pod
// -> all-gather -> windows + this shard's records -> all-gather -> chain +
// pairs (s.pmax: [M | broken]) -> all-reduce (max) -> commit
void launch_adapt_sh_mask(const LaunchArgs& a, uint64_t* send, int32_t W, hipStream_t stream);
void launch_adapt_sh_window(const LaunchArgs& a, const uint64_t* recv, int32_t W, uint64_t* gmask, hipStream_t stream);
void launch_adapt_sh_pairs(const LaunchArgs& a, const uint64_t* gmask, int32_t world, hipStream_t stream);
void launch_adapt_sh_commit(const LaunchArgs& a, hipStream_t stream);
void launch_shard_chain(const LaunchArgs& a, int32_t world, hipStream_t stream);
void launch_shard_commit(const LaunchArgs& a, hipStream_t stream);
// Sharded per-pod cycle (node shards; the caller exchanges between the phases,
// see ksim_kernels.hip §C):
//   launch_pshard_topo     prefilter + pack           (all-reduce sum s.xdom)
//   launch_pshard_filter   [topo min] + filter + counts (all-gather s.xsend[2] -> s.xrecv[world][2])
//   launch_pshard_window   cut / kept / registrations (all-reduce sum s.xreg; pods with soft spread)
//   launch_pshard_extrema  weights + extrema            (all-reduce max win->ext[kExtWords])
//   launch_pshard_select   totals + TB pair, shard best  (all-gather s.xsend[2] -> s.xrecv[world][2])
//   launch_pshard_bind     selectHost over the shards, owner binds
void launch_pshard_topo(const LaunchArgs& a, hipStream_t stream);
void launch_pshard_filter(const LaunchArgs& a, bool topo, hipStream_t stream);
void launch_pshard_window(const LaunchArgs& a, int32_t rank, int32_t world, hipStream_t stream);
void launch_pshard_extrema(const LaunchArgs& a, bool soft, hipStream_t stream);
void launch_pshard_select(const LaunchArgs& a, hipStream_t stream);
void launch_pshard_bind(const LaunchArgs& a, int32_t world, hipStream_t stream);
void launch_group_reduce(const GroupPtrs& g, int64_t count, bool op_max, hipStream_t stream);
void launch_group_gather(const GroupPtrs& src, const GroupPtrs& dst, int32_t words, hipStream_t stream);
// Persistent domain tables of a loaded queue (DevPods.ptab) from the class counts.
void launch_ptab_init(const DevCluster& c, const DevPods& P, hipStream_t stream);
// ksim_reset_cluster: copies (or zeroes, src null) of 16-byte-aligned buffers in one launch
struct ResetList {
  static constexpr int kMax = 12;
  int n = 0;
  uint32_t* dst[kMax];
  const uint32_t* src[kMax];
  size_t words[kMax];
  // Takes the entry when k_reset_copy can (a slot left, whole words, both
  // pointers 16-byte aligned: it moves uint4 words); false: the caller copies
  // it itself.
  [[nodiscard]] bool add(void* d, const void* s, size_t bytes) {
    if (n >= kMax || bytes % 4 != 0 || ((uintptr_t)d & 15) != 0 || ((uintptr_t)s & 15) != 0) return false;
    dst[n] = (uint32_t*)d;
    src[n] = (const uint32_t*)s;
    words[n] = bytes / 4;
    n++;
    return true;
  }
};
void launch_reset_copy(const ResetList& L, hipStream_t stream);
// run_lazy's begin and end in one launch each (k_lazy_move): the six dynamic
// columns dst = src by element (any n, any alignment) and the state.
// begin: st_dst and st_dst2 receive st_src with the run header (first, end),
// bcap zeroed and, zero_counters set, the call's counters zeroed; the window
// state zeroed, every ring slot emptied and the batch counter the run starts
// from stored to *batches0 (the progress word's base, host-mapped).
// End (begin = 0): st_dst = st_src.
struct LazyMove {
  DynCols src, dst;
  int32_t n;
  int32_t begin, zero_counters, first, end;
  const DevState* st_src;
  DevState* st_dst;
  DevState* st_dst2;
  WinState* win;
  int32_t* ring_e;                                 // [kLazySlots]
  unsigned long long* batches0;
};
void launch_lazy_move(const LazyMove& m, hipStream_t stream);

// Selector / term matching as an int8 contraction (ksim_match.hip, ksim_match_terms).
constexpr int kMatchMaxReqs = 4096;     // requirement columns (LDS: 16 rows x 4096 bits)
constexpr int kMatchMaxFeat = 65536;    // feature vocabulary (K of the contraction)
struct DevMatch {
  const int8_t* a;          // [sp][fp] signature one-hot rows (zeroed before the scatter)
  const int8_t* bt;         // [rp][fp] requirement rows (B transposed)
  const uint8_t* neg;       // [rp] 1: satisfied when no feature hits
  const int32_t *sig_off, *sig_feat, *req_off, *req_feat;   // CSR feature lists
  const int32_t *m_off, *m_req;                               // CSR requirement lists per matcher
  const int32_t *pod_sig, *pod_node, *cls_matcher;
  uint32_t* bits;           // [s][w] matcher bits per signature
  uint32_t* cls_bits;       // [s][cw] class bits per signature
  int32_t* cnt;             // [c][n] class counts over the bound pods (zeroed)
  int32_t s, sp, fp, r, rp, m, w, c, cw, p, n;
};
void launch_match(const DevMatch& m, hipStream_t stream);
void launch_assume(const DevCluster& c, const DevPods& P, int32_t pod, int32_t node, int sign, hipStream_t stream);

}  // namespace ksim
