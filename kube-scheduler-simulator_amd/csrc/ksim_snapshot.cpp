// ksim_snapshot.cpp — the node snapshot's life cycle behind the C ABI:
// ksim_set_cluster, the node informer deltas (ksim_upsert_nodes,
// ksim_update_node_rows, ksim_remove_node), ksim_reset_cluster, the volume
// limit table and the state getters and setters.  The dynamic columns, the
// cluster facts and the teardowns are each said once here (for_dyn_cols,
// cluster_facts), in ksim_engine.cpp (drop_loaded_pods) or are an assignment
// of a fresh value to a struct of the handle (ksim_host.h BoundPods, LazyBufs).
#include <algorithm>
#include <cstring>
#include <type_traits>

#include "ksim_host.h"

using namespace ksim_host;

namespace {

// One dynamic node column: the live array the cycles' binds change (h->dc),
// its copy as last uploaded (h->init), the ksim_node_table column it comes
// from and its arrays of n values (1, n_scalar, n_classes).
template <class T>
struct DynCol {
  using value_type = T;
  T*& live;
  T*& snap;
  const T* ksim_node_table::*field;   // null: no table column (the volume attachment counts)
  const T* tab;                       // that column of the table handed to for_dyn_cols (null without one)
  int32_t rows;                       // of the handle's snapshot
  int32_t tab_rows;                   // of the table
};

// The dynamic columns, each once, in ksim_reset_cluster's order: the one list
// behind the snapshot copy, the node deltas' replay and the reset.  The volume
// attachment counts (ksim_set_volume_limits owns their buffers) are listed
// while a volume table is set, which the node deltas refuse.
template <class F>
int for_dyn_cols(ksim_handle* h, const ksim_node_table* t, F&& f) {
  DevCluster& c = h->dc;
  auto& s = h->init;
  auto col = [&](auto*& live, auto*& snap, auto field, int32_t rows, int32_t tab_rows) {
    using T = typename std::remove_reference<decltype(*live)>::type;
    return f(DynCol<T>{live, snap, field, t && field ? t->*field : nullptr, rows, t ? tab_rows : 0});
  };
  using Tab = ksim_node_table;
  const int32_t ts = t ? t->n_scalar : 0, tc = t ? t->n_classes : 0;
  int rc;
  if ((rc = col(c.req_cpu, s.req_cpu, &Tab::req_cpu, 1, 1)) ||
      (rc = col(c.req_mem, s.req_mem, &Tab::req_mem, 1, 1)) ||
      (rc = col(c.req_eph, s.req_eph, &Tab::req_eph, 1, 1)) ||
      (rc = col(c.req_scalar, s.req_scalar, &Tab::req_scalar, c.n_scalar, ts)) ||
      (rc = col(c.nz_cpu, s.nz_cpu, &Tab::nz_cpu, 1, 1)) ||
      (rc = col(c.nz_mem, s.nz_mem, &Tab::nz_mem, 1, 1)) ||
      (rc = col(c.num_pods, s.num_pods, &Tab::num_pods, 1, 1)) ||
      (rc = col(c.cnt, s.cnt, &Tab::class_count, c.n_classes, tc)) ||
      (rc = col(c.nb_alloc, s.nb_alloc, &Tab::nb_alloc, 1, 1)))
    return rc;
  if (c.vol_nf) return col(c.vol_attached, h->vol_init, (const int32_t* Tab::*)nullptr, c.vol_nf, 0);
  return KSIM_OK;
}

// The cluster facts the filter plans read, from the whole table: the hard
// taints some node carries, unschedulable nodes, narrow allocatable (the
// handle's host copies and the returned DevCluster::cflags), and per label
// column whether every node carries the key (h->col_total) and whether every
// value sits on at most one node (uniq, hostname: InterPodAffinity reads the
// node's own count there, kUseUniqueCol; all zero on shard handles, whose
// domain sums are exchanged as tables).  The caller uploads uniq.
uint32_t cluster_facts(ksim_handle* h, const ksim_node_table* t, const ksim_vocab* v,
                       const std::vector<int32_t>& col_nvals, std::vector<uint8_t>& uniq) {
  const int32_t n = t->n_nodes;
  const size_t N = (size_t)n;
  std::vector<uint8_t> seen((size_t)v->n_taints, 0);
  for (size_t i = 0; i < N * KSIM_MAX_NODE_TAINTS; i++) seen[t->taints[i]] = 1;
  h->hard_taints.clear();
  for (int id = 1; id < v->n_taints; id++)
    if (seen[id] && (v->taint_effect[id] == KSIM_EFFECT_NO_SCHEDULE || v->taint_effect[id] == KSIM_EFFECT_NO_EXECUTE))
      h->hard_taints.push_back((uint16_t)id);
  h->any_unschedulable = false;
  for (int32_t i = 0; i < n; i++) h->any_unschedulable = h->any_unschedulable || (t->flags[i] & KSIM_NODE_UNSCHEDULABLE);
  uint32_t cf = h->any_unschedulable ? kClusterUnschedulable : 0u;
  if (!h->hard_taints.empty()) cf |= kClusterHardTaints;
  for (size_t i = 0; i < N * KSIM_MAX_NODE_TAINTS; i++)
    if (t->taints[i] && v->taint_effect[t->taints[i]] == KSIM_EFFECT_PREFER_NO_SCHEDULE) cf |= kClusterPreferTaints;
  h->alloc_narrow = true;
  for (int32_t i = 0; i < n; i++)
    h->alloc_narrow = h->alloc_narrow && t->alloc_cpu[i] >= 0 && t->alloc_cpu[i] < (1ll << 46) &&
                      t->alloc_mem[i] >= 0 && t->alloc_mem[i] < (1ll << 46);
  if (h->alloc_narrow) cf |= kClusterNarrow;
  uniq.assign((size_t)t->n_label_cols, 0);
  h->col_total.assign((size_t)t->n_label_cols, 1);
  std::vector<uint8_t> vs;
  for (int k = 0; k < t->n_label_cols; k++) {
    vs.assign((size_t)col_nvals[k], 0);
    bool u = !h->shard_total;
    for (int32_t i = 0; i < n; i++) {
      const uint32_t x = t->labels[(size_t)k * N + i];
      if (!x) h->col_total[k] = 0;
      if (x && vs[x]++) u = false;
    }
    uniq[k] = u;
  }
  return cf;
}

}  // namespace

int ksim_set_cluster(ksim_handle* h, const ksim_node_table* t, const ksim_vocab* v) {
  if (const int prc = flush_pend_bind(h)) return prc;   // a queued Reserve lands first
  if (!h || !t || !v) return KSIM_E_INVALID;
  h->stab_dirty = true;
  HIPCHK(h, hipSetDevice(h->device));
  const int32_t n = t->n_nodes;
  if (n < 0 || n > KSIM_MAX_NODES) return set_err(h, KSIM_E_INVALID, "n_nodes out of range");
  if (t->n_scalar < 0 || t->n_scalar > KSIM_MAX_SCALAR) return set_err(h, KSIM_E_INVALID, "n_scalar out of range");
  if (t->n_label_cols < 0 || t->n_label_cols > KSIM_MAX_LABEL_COLS)
    return set_err(h, KSIM_E_INVALID, "n_label_cols out of range");
  if (v->n_taints < 1 || v->n_taints > 64 * KSIM_TAINT_WORDS || !v->taint_effect)
    return set_err(h, KSIM_E_INVALID, "n_taints out of range");
  if (n > 0 && (!t->alloc_cpu || !t->alloc_mem || !t->alloc_eph || !t->alloc_pods || !t->req_cpu || !t->req_mem ||
                !t->req_eph || !t->nz_cpu || !t->nz_mem || !t->num_pods || !t->flags || !t->taints ||
                (t->n_label_cols > 0 && !t->labels) || (t->n_scalar > 0 && (!t->alloc_scalar || !t->req_scalar))))
    return set_err(h, KSIM_E_INVALID, "null node column");
  for (size_t i = 0; i < (size_t)n * KSIM_MAX_NODE_TAINTS; i++)
    if (t->taints[i] >= v->n_taints) return set_err(h, KSIM_E_INVALID, "taint id out of vocabulary");
  if (t->n_label_cols > 0 && (!v->label_col_offset || (v->n_label_values > 0 && (!v->label_num || !v->label_num_ok))))
    return set_err(h, KSIM_E_INVALID, "null label vocabulary");
  // value ids per label column: every label id must index its column's domain
  // tables (device atomics use it as an address)
  std::vector<int32_t> col_nvals((size_t)t->n_label_cols, 0);
  int32_t vmax = 1;
  for (int k = 0; k < t->n_label_cols; k++) {
    const int32_t end = k + 1 < t->n_label_cols ? v->label_col_offset[k + 1] : v->n_label_values;
    col_nvals[k] = end - v->label_col_offset[k];
    if (v->label_col_offset[k] < 0 || col_nvals[k] < 1 || end > v->n_label_values)
      return set_err(h, KSIM_E_INVALID, "label_col_offset not increasing within n_label_values");
    if (col_nvals[k] > KSIM_MAX_NODES + 1) return set_err(h, KSIM_E_INVALID, "label column vocabulary too large");
    vmax = std::max(vmax, col_nvals[k]);
    for (int32_t i = 0; i < n; i++)
      if (t->labels[(size_t)k * n + i] >= (uint32_t)col_nvals[k])
        return set_err(h, KSIM_E_INVALID, "label value id out of its column's vocabulary");
  }
  if (t->n_classes < 0 || t->n_classes > KSIM_MAX_CLASSES || (t->n_classes > 0 && n > 0 && !t->class_count))
    return set_err(h, KSIM_E_INVALID, "n_classes out of range / null class_count");
  if (v->n_topo_log < 0 || (v->n_topo_log > 0 && !v->topo_log))
    return set_err(h, KSIM_E_INVALID, "bad topo_log");
  (void)hipStreamSynchronize(h->stream);
  // the inputs are valid: the old snapshot goes, and with it the evaluation
  // range (a replica calls ksim_set_eval_range again)
  h->replicated = false;
  drop_graphs(h);
  h->cluster_bufs.clear();
  h->vol_bufs.clear();               // the volume table belongs to the old snapshot (DevCluster c{} below)
  h->vol_init = nullptr;
  h->scratch_bufs.clear();
  h->ash = AshBufs{};
  h->lazy = LazyBufs{};
  drop_loaded_pods(h);                  // d_chosen with it
  h->has_cluster = false;
  // node positions of the old snapshot: the bound-pod table and a pending
  // extender round trip do not carry over
  h->bound = BoundPods{};
  h->ext_pending = false;
  h->fw_pending = h->fw_scored = h->fw_dom_dirty = false;   // fresh scratch below
  h->deferred_binds.clear();           // Reserve / Unreserve queued against the old node positions

  const int32_t n_total = h->shard_total ? h->shard_total : n;
  if (h->shard_base < 0 || h->shard_base + n > n_total || n_total > KSIM_MAX_NODES)
    return set_err(h, KSIM_E_INVALID, "shard range outside the cluster (ksim_set_shard)");
  DevCluster c{};
  c.count_whole = 1;
  c.base = h->shard_base;
  c.n_total = n_total;
  c.n_classes = t->n_classes;
  c.n_topo_log = v->n_topo_log;
  c.vmax = vmax;
  c.n = n;
  c.n_scalar = t->n_scalar;
  c.n_label_cols = t->n_label_cols;
  c.n_taints = v->n_taints;
  c.n_label_values = v->n_label_values;
  const size_t N = (size_t)n;
  int rc;
  auto up = [&](auto*& dst, const void* src, size_t bytes) { return h->cluster_bufs.alloc(h, dst, bytes, src); };
  // label columns whose every value sits on at most one node (hostname):
  // InterPodAffinity reads the node's own count there (kUseUniqueCol)
  std::vector<uint8_t> uniq;
  c.cflags = cluster_facts(h, t, v, col_nvals, uniq);
  std::vector<double> ic(N), im(N);                    // RN(1 / allocatable): IEEE division on the host
  for (size_t i = 0; i < N; i++) {
    ic[i] = t->alloc_cpu[i] ? 1.0 / (double)t->alloc_cpu[i] : 0.0;
    im[i] = t->alloc_mem[i] ? 1.0 / (double)t->alloc_mem[i] : 0.0;
  }
  if ((rc = up(c.alloc_cpu, t->alloc_cpu, 8 * N)) ||
      (rc = up(c.alloc_mem, t->alloc_mem, 8 * N)) ||
      (rc = up(c.alloc_eph, t->alloc_eph, 8 * N)) ||
      (rc = up(c.alloc_pods, t->alloc_pods, 4 * N)) ||
      (rc = up(c.alloc_scalar, t->alloc_scalar, 8 * N * t->n_scalar)) ||
      (rc = up(c.req_cpu, t->req_cpu, 8 * N)) ||
      (rc = up(c.req_mem, t->req_mem, 8 * N)) ||
      (rc = up(c.req_eph, t->req_eph, 8 * N)) ||
      (rc = up(c.req_scalar, t->req_scalar, 8 * N * t->n_scalar)) ||
      (rc = up(c.nz_cpu, t->nz_cpu, 8 * N)) ||
      (rc = up(c.nz_mem, t->nz_mem, 8 * N)) ||
      (rc = up(c.num_pods, t->num_pods, 4 * N)) ||
      (rc = up(c.flags, t->flags, 4 * N)) ||
      (rc = up(c.taints, t->taints, 2 * N * KSIM_MAX_NODE_TAINTS)) ||
      (rc = up(c.labels, t->labels, 4 * N * t->n_label_cols)) ||
      (rc = up(c.taint_effect, v->taint_effect, (size_t)v->n_taints)) ||
      (rc = up(c.label_col_offset, v->label_col_offset, 4 * (size_t)t->n_label_cols)) ||
      (rc = up(c.label_num, v->label_num, 8 * (size_t)std::max(v->n_label_values, 0))) ||
      (rc = up(c.label_num_ok, v->label_num_ok, (size_t)std::max(v->n_label_values, 0))) ||
      (rc = up(c.cnt, t->class_count, 4 * N * (size_t)t->n_classes)) ||
      (rc = up(c.topo_log, v->topo_log, 8 * (size_t)v->n_topo_log)) ||
      (rc = up(c.col_nvals, col_nvals.data(), 4 * col_nvals.size())) ||
      (rc = up(c.col_unique, uniq.data(), uniq.size())) ||
      (rc = up(c.nb_limit, t->nb_limit, 8 * N)) ||       // zeros when no node has the annotation
      (rc = up(c.nb_alloc, t->nb_alloc, 8 * N)) ||
      (rc = up(c.inv_cpu, ic.data(), 8 * N)) ||
      (rc = up(c.inv_mem, im.data(), 8 * N)))
    return rc;
  h->col_unique = uniq;
  h->col_nvals = col_nvals;
  c.fit_ignore = h->has_profile ? h->prof.fit_ignored_scalar : 0u;
  h->dc = c;
  h->taint_effect.assign(v->taint_effect, v->taint_effect + v->n_taints);
  // the dynamic columns as uploaded: what ksim_reset_cluster restores
  rc = for_dyn_cols(h, nullptr, [&](auto col) -> int {
    const size_t bytes = sizeof(*col.live) * N * (size_t)col.rows;
    if (const int r = h->cluster_bufs.alloc(h, col.snap, bytes)) return r;
    HIPCHK(h, hipMemcpyAsync(col.snap, col.live, bytes, hipMemcpyDeviceToDevice, h->stream));
    return KSIM_OK;
  });
  if (rc) return rc;

  DevScratch s{};
  DevEvalOut o{};
  auto scr = [&](auto*& dst, size_t bytes) { return h->scratch_bufs.alloc(h, dst, bytes); };
  const size_t NT = N <= (size_t)kTbMaxBlocks * 256 ? N : 0;   // topology batches (tbatch_admit)
  const size_t NW = (N + 63) / 64 <= 128 ? N : 0;   // the doubling window's tables (clusters of <= 128 bitmap words)
  if ((rc = scr(s.fail, N)) ||
      (rc = scr(s.ign, N)) ||
      (rc = scr(s.win, sizeof(WinState))) ||
      (rc = scr(s.bbest, 16 * ((N + 255) / 256))) ||
      (rc = scr(s.regbm, 4 * (size_t)KSIM_MAX_USES * ((vmax + 31) / 32))) ||
      (rc = scr(h->ext_fail, N)) ||
      (rc = scr(h->ext_score, 8 * N)) ||
      (rc = scr(h->fw_nodes, 4 * N)) ||
      (rc = scr(h->fw_vals, 8 * N)) ||
      (rc = scr(h->fw_out, 8 * N)) ||
      (rc = scr(s.detail, 4 * N)) ||
      (rc = scr(s.raw, 8 * N * KSIM_MAX_SCORE)) ||
      (rc = scr(s.part, 8 * N)) ||
      // [B][kMaxListRecords] list records: the node-stationary evaluation writes one per node slice
      (rc = scr(s.topk, 8 * (size_t)kBatchPods * kMaxListRecords * kTopT)) ||
      (rc = scr(s.topk_cnt, 4 * (size_t)kBatchPods * kMaxListRecords)) ||
      (rc = scr(s.topk_complete, 4 * (size_t)kBatchPods * kMaxListRecords)) ||
      (rc = scr(s.gkey, 8 * (size_t)kBatchPods)) ||
      (rc = scr(s.chain_end, 4)) ||
      (rc = scr(s.pmax, 8 * 2 * (size_t)kBatchPods)) ||   // [M | sharded ADAPT broken flags]
      (rc = scr(s.pnorm, 8 * 4 * (size_t)kBatchPods)) ||
      (rc = scr(s.tb_fail, (size_t)kTbPods * NT)) ||
      (rc = scr(s.tb_ign, (size_t)kTbPods * NT)) ||
      (rc = scr(s.tb_part, 8 * (size_t)kTbPods * NT)) ||
      (rc = scr(s.tb_raw, 8 * (size_t)kTbPods * KSIM_MAX_SCORE * NT)) ||
      (rc = scr(s.tb_stat, 4 * (size_t)kTbPods * kVarSlots * NT)) ||   // per zone-variant slot
      (rc = scr(s.tb_win, sizeof(WinState) * (size_t)kTbPods)) ||
      (rc = scr(s.tb_var, sizeof(TbVar) * (size_t)kTbPods)) ||
      (rc = scr(s.tb_dom, sizeof(TbDom) * (size_t)kTbPods * kVarDom)) ||
      (rc = scr(s.tb_vhold, 4 * (size_t)kTbPods * kVarSlots * 2 * KSIM_MAX_SCORE)) ||
      (rc = scr(s.tb_slot, 4 * (size_t)kTbPods)) ||
      (rc = scr(s.tb_vdom, (size_t)kTbPods * NT)) ||
      (rc = scr(s.tb_cdom, (size_t)kTbPods * kVarSlots * kTbMaxBlocks * kTopT)) ||
      (rc = scr(s.tb_kdom, (size_t)kTbPods * kVarSlots * kTopT)) ||
      (rc = scr(s.tb_vnf, 4 * (size_t)kTbPods * kVarSlots)) ||
      (rc = scr(s.tb_vpods, 8)) ||
      (rc = scr(s.tb_clist, 8 * (size_t)kTbPods * kVarSlots * kTbMaxBlocks * kTopT)) ||
      (rc = scr(s.tb_ccnt, 4 * (size_t)kTbPods * kVarSlots * kTbMaxBlocks)) ||
      (rc = scr(s.tb_xrecv, sizeof(WinState) * (size_t)kMaxShards * kTbPods)) ||
      (rc = scr(s.tb_pp, 8 * 2 * (size_t)kTbPods)) ||
      (rc = scr(s.pinv, 4 * (size_t)kBatchPods)) ||
      (rc = scr(s.dom, 8 * (size_t)KSIM_MAX_USES * vmax)) ||
      (rc = scr(s.dbg, 8 * 16)) ||
      (rc = scr(s.xsend, 8 * (size_t)kBatchPods * kXRec)) ||
      (rc = scr(s.xrecv, 8 * (size_t)kMaxShards * kBatchPods * kXRec)) ||
      (rc = scr(s.min_match, 8 * (size_t)KSIM_MAX_USES)) ||
      (rc = scr(s.xdom, 8 * (size_t)KSIM_MAX_USES * vmax)) ||
      (rc = scr(s.amask, 8 * (size_t)kBatchPods * ((N + 63) / 64))) ||
      (rc = scr(s.awin, 4 * 2 * (size_t)kBatchPods)) ||
      (rc = scr(s.aexact, 4)) ||
      (rc = scr(s.acut, 4 * 2 * (size_t)kBatchPods)) ||
      (rc = scr(s.wtab, 2 * 3 * (size_t)kBatchPods * std::max<size_t>(NW, 1))) ||
      (rc = scr(s.wtot, 4 * (size_t)kBatchPods)) ||
      (rc = scr(s.abroken, 4 * (size_t)kBatchPods)) ||
      (rc = scr(s.xreg, 8 * (1 + (size_t)KSIM_MAX_USES * vmax))) ||
      (rc = scr(o.scored, N)) ||
      (rc = scr(o.raw, 8 * N * KSIM_MAX_SCORE)) ||
      (rc = scr(o.norm, 8 * N * KSIM_MAX_SCORE)) ||
      (rc = scr(o.total, 8 * N)))
    return rc;
  h->sc = s;
  h->eo = o;
  DevState zero{};
  HIPCHK(h, hipMemcpyAsync(h->st, &zero, sizeof(zero), hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->has_cluster = true;
  return KSIM_OK;
}

// Node informer deltas: the new table in nodeTree order, old_pos[i] = the
// current position of new node i or -1 (added).  The table is the new
// snapshot (static columns, vocabulary and the dynamic columns of the bound
// pods); on a kept node the binds the cycles made since the last snapshot
// (device column - snapshot column at old_pos) are replayed on top of it, for
// every scalar column / count class the handle already has.  nextStartNodeIndex
// carries over mod the new node count (upstream keeps the index and scans
// nodes[(index + i) % numAllNodes]), and so does the tie-break sequence.
// Loaded pods, the bound-pod table and captured graphs are dropped (node
// positions changed).
int ksim_upsert_nodes(ksim_handle* h, const ksim_node_table* t, const ksim_vocab* v, const int32_t* old_pos) {
  if (const int prc = flush_pend_bind(h)) return prc;   // a queued Reserve lands first
  // (a replica keeps its flag when the delta is refused; the new snapshot
  // below clears it: ksim_set_eval_range again)
  if (!h || !t || !v) return KSIM_E_INVALID;
  h->stab_dirty = true;
  if (!h->has_cluster) return set_err(h, KSIM_E_INVALID, "ksim_upsert_nodes before ksim_set_cluster");
  if (h->shard_total || h->world > 1) return set_err(h, KSIM_E_UNSUPPORTED, "ksim_upsert_nodes on a shard handle");
  if (h->dc.vol_nf)
    return set_err(h, KSIM_E_UNSUPPORTED, "ksim_upsert_nodes while a volume table is set (send the snapshot and "
                                          "ksim_set_volume_limits again)");
  HIPCHK(h, hipSetDevice(h->device));
  const int32_t n = t->n_nodes, n0 = h->dc.n;
  if (n < 0 || n > KSIM_MAX_NODES) return set_err(h, KSIM_E_INVALID, "n_nodes out of range");
  if (n > 0 && !old_pos) return set_err(h, KSIM_E_INVALID, "null old_pos");
  const int32_t s0 = h->dc.n_scalar, c0 = h->dc.n_classes;
  if (t->n_scalar < s0 || t->n_scalar > KSIM_MAX_SCALAR)
    return set_err(h, KSIM_E_INVALID, "scalar columns may only be appended");
  if (t->n_classes < c0 || t->n_classes > KSIM_MAX_CLASSES)
    return set_err(h, KSIM_E_INVALID, "count classes may only be appended");
  if (n > 0 && (!t->req_cpu || !t->req_mem || !t->req_eph || !t->nz_cpu || !t->nz_mem || !t->num_pods ||
                (t->n_scalar > 0 && !t->req_scalar) || (t->n_classes > 0 && !t->class_count)))
    return set_err(h, KSIM_E_INVALID, "null node column");
  {
    std::vector<uint8_t> seen((size_t)n0, 0);
    for (int32_t i = 0; i < n; i++) {
      const int32_t op = old_pos[i];
      if (op < -1 || op >= n0 || (op >= 0 && seen[op]++))
        return set_err(h, KSIM_E_INVALID, "old_pos: out of range or repeated");
    }
  }
  HIPCHK(h, hipStreamSynchronize(h->stream));
  DevState st{};
  HIPCHK(h, hcopy(h, &st, h->st, sizeof(st), hipMemcpyDeviceToHost));
  const size_t N = (size_t)n, N0 = (size_t)n0;
  // per dynamic column: out = table + (device - snapshot) at old_pos, rows of n0 -> rows of n
  std::vector<std::vector<char>> outs;
  int rc = for_dyn_cols(h, t, [&](auto col) -> int {
    using T = typename decltype(col)::value_type;
    const size_t rows = (size_t)col.tab_rows, rows0 = (size_t)col.rows;
    std::vector<T> a(N0 * rows0), b(N0 * rows0);
    if (!a.empty()) {
      HIPCHK(h, hcopy(h, a.data(), col.live, sizeof(T) * a.size(), hipMemcpyDeviceToHost));
      HIPCHK(h, hcopy(h, b.data(), col.snap, sizeof(T) * b.size(), hipMemcpyDeviceToHost));
    }
    outs.emplace_back(sizeof(T) * N * rows);
    T* out = (T*)outs.back().data();
    for (size_t k = 0; k < rows; k++)
      for (size_t i = 0; i < N; i++) {
        T x = col.tab ? col.tab[k * N + i] : 0;
        if (k < rows0 && old_pos[i] >= 0) x += a[k * N0 + old_pos[i]] - b[k * N0 + old_pos[i]];
        out[k * N + i] = x;
      }
    return KSIM_OK;
  });
  if (rc) return rc;
  // the table becomes the snapshot (ksim_set_cluster copies it to h->init)
  if ((rc = ksim_set_cluster(h, t, v)) != KSIM_OK) return rc;
  size_t next = 0;
  rc = for_dyn_cols(h, nullptr, [&](auto col) -> int {
    const std::vector<char>& out = outs[next++];
    if (!out.empty()) HIPCHK(h, hcopy(h, col.live, out.data(), out.size(), hipMemcpyHostToDevice));
    return KSIM_OK;
  });
  if (rc) return rc;
  DevState s2{};
  s2.next_start = n > 0 ? st.next_start % n : 0;
  s2.pod_seq = st.pod_seq;
  HIPCHK(h, hcopy(h, h->st, &s2, sizeof(s2), hipMemcpyHostToDevice));
  return KSIM_OK;
}

// UpdateNode in place: the changed rows' static columns through one launch
// from the pinned staging; the cluster facts the filter plans read (hard
// taints, unschedulable nodes, narrow allocatable, unique / total label
// columns) recomputed from the whole table on the host.
int ksim_update_node_rows(ksim_handle* h, const ksim_node_table* t, const ksim_vocab* v, const int32_t* rows,
                          int32_t n_rows) {
  if (const int prc = flush_pend_bind(h)) return prc;   // a queued Reserve lands first
  if (!h || !t || !v || n_rows < 0 || (n_rows > 0 && !rows)) return KSIM_E_INVALID;
  if (!h->has_cluster) return set_err(h, KSIM_E_INVALID, "ksim_update_node_rows before ksim_set_cluster");
  if (h->shard_total || h->world > 1) return set_err(h, KSIM_E_UNSUPPORTED, "ksim_update_node_rows on a shard handle");
  if (h->dc.vol_nf)
    return set_err(h, KSIM_E_UNSUPPORTED, "ksim_update_node_rows while a volume table is set (send the snapshot and "
                                          "ksim_set_volume_limits again)");
  const DevCluster& c = h->dc;
  const int32_t n = c.n;
  if (t->n_nodes != n || t->n_scalar != c.n_scalar || t->n_label_cols != c.n_label_cols ||
      t->n_classes != c.n_classes || v->n_taints != c.n_taints || v->n_label_values != c.n_label_values)
    return set_err(h, KSIM_E_INVALID, "ksim_update_node_rows: the table's layout or vocabulary differs (ksim_upsert_nodes)");
  if (n > 0 && (!t->alloc_cpu || !t->alloc_mem || !t->alloc_eph || !t->alloc_pods || !t->flags || !t->taints ||
                (t->n_label_cols > 0 && !t->labels) || (t->n_scalar > 0 && !t->alloc_scalar)))
    return set_err(h, KSIM_E_INVALID, "null node column");
  for (int k = 0; k < c.n_label_cols; k++)
    if (!v->label_col_offset || (k + 1 < c.n_label_cols ? v->label_col_offset[k + 1] : v->n_label_values) -
                                        v->label_col_offset[k] != h->col_nvals[k])
      return set_err(h, KSIM_E_INVALID, "ksim_update_node_rows: a label column's vocabulary changed (ksim_upsert_nodes)");
  if (!v->taint_effect || !std::equal(h->taint_effect.begin(), h->taint_effect.end(), v->taint_effect))
    return set_err(h, KSIM_E_INVALID, "ksim_update_node_rows: the taint vocabulary changed (ksim_upsert_nodes)");
  const size_t N = (size_t)n;
  std::vector<uint8_t> seen_row((size_t)n, 0);
  for (int32_t q = 0; q < n_rows; q++) {
    const int32_t r = rows[q];
    if (r < 0 || r >= n || seen_row[r]++) return set_err(h, KSIM_E_INVALID, "rows: out of range or repeated");
    for (int k = 0; k < KSIM_MAX_NODE_TAINTS; k++)
      if (t->taints[(size_t)k * N + r] >= v->n_taints) return set_err(h, KSIM_E_INVALID, "taint id out of vocabulary");
    for (int k = 0; k < c.n_label_cols; k++)
      if (t->labels[(size_t)k * N + r] >= (uint32_t)h->col_nvals[k])
        return set_err(h, KSIM_E_INVALID, "label value id out of its column's vocabulary");
  }
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));     // the pinned staging is free
  const int32_t words = 1 + 8 + KSIM_MAX_NODE_TAINTS + c.n_scalar + c.n_label_cols;
  int rc;
  if ((rc = h->pin.reserve(h, 8 * (size_t)words * (size_t)std::max(n_rows, 1), Idle::kCaller))) return rc;   // idle: drained above
  int64_t* rec = (int64_t*)h->pin.p;
  for (int32_t q = 0; q < n_rows; q++) {
    const int32_t r = rows[q];
    int64_t* w = rec + (size_t)q * words;
    const double ic = t->alloc_cpu[r] ? 1.0 / (double)t->alloc_cpu[r] : 0.0;   // as ksim_set_cluster
    const double im = t->alloc_mem[r] ? 1.0 / (double)t->alloc_mem[r] : 0.0;
    w[0] = r;
    w[1] = t->alloc_cpu[r];
    w[2] = t->alloc_mem[r];
    w[3] = t->alloc_eph[r];
    w[4] = t->alloc_pods[r];
    w[5] = t->flags[r];
    w[6] = t->nb_limit ? t->nb_limit[r] : 0;
    std::memcpy(&w[7], &ic, 8);
    std::memcpy(&w[8], &im, 8);
    for (int k = 0; k < KSIM_MAX_NODE_TAINTS; k++) w[9 + k] = t->taints[(size_t)k * N + r];
    for (int k = 0; k < c.n_scalar; k++) w[9 + KSIM_MAX_NODE_TAINTS + k] = t->alloc_scalar[(size_t)k * N + r];
    for (int k = 0; k < c.n_label_cols; k++)
      w[9 + KSIM_MAX_NODE_TAINTS + c.n_scalar + k] = t->labels[(size_t)k * N + r];
  }
  launch_node_rows(c, (const int64_t*)h->pin.d, n_rows, words, h->stream);
  HIPCHK(h, hipGetLastError());
  // the cluster facts, from the whole table
  std::vector<uint8_t> uniq;
  h->dc.cflags = cluster_facts(h, t, v, h->col_nvals, uniq);
  if (uniq != h->col_unique && c.n_label_cols > 0) {
    HIPCHK(h, hcopy(h, const_cast<uint8_t*>(c.col_unique), uniq.data(), uniq.size(), hipMemcpyHostToDevice));
    h->col_unique = uniq;
  }
  // what was compiled against the old rows: graphs, the static-class table, loaded pods
  drop_graphs(h);
  h->stab_dirty = true;
  drop_loaded_pods(h);
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return KSIM_OK;
}

// DeleteNode: the node at `pos` leaves; later positions move down by one.  The
// table handed to ksim_upsert_nodes is the current snapshot without it, so the
// replay keeps every other node's state.
int ksim_remove_node(ksim_handle* h, int32_t pos) {
  if (const int prc = flush_pend_bind(h)) return prc;   // a queued Reserve lands first
  if (!h || !h->has_cluster) return set_err(h, KSIM_E_INVALID, "cluster not set");
  h->stab_dirty = true;
  if (h->shard_total || h->world > 1) return set_err(h, KSIM_E_UNSUPPORTED, "ksim_remove_node on a shard handle");
  if (h->dc.vol_nf)
    return set_err(h, KSIM_E_UNSUPPORTED, "ksim_remove_node while a volume table is set (send the snapshot and "
                                          "ksim_set_volume_limits again)");
  const int32_t n0 = h->dc.n;
  if (pos < 0 || pos >= n0) return set_err(h, KSIM_E_INVALID, "node position out of range");
  h->replicated = false;                        // a new snapshot: ksim_set_eval_range again
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  const DevCluster& c = h->dc;
  const int32_t n = n0 - 1;
  const size_t N0 = (size_t)n0;
  // the static columns and vocabulary, read back and compacted
  auto pull = [&](auto& out, const auto* dev, size_t rows) -> int {
    using T = typename std::remove_reference<decltype(out)>::type::value_type;
    std::vector<T> all(N0 * rows);
    if (!all.empty()) HIPCHK(h, hcopy(h, all.data(), dev, sizeof(T) * all.size(), hipMemcpyDeviceToHost));
    out.clear();
    for (size_t k = 0; k < rows; k++)
      for (size_t i = 0; i < N0; i++)
        if ((int32_t)i != pos) out.push_back(all[k * N0 + i]);
    return KSIM_OK;
  };
  std::vector<int64_t> ac, am, ae, as, nbl;
  std::vector<int32_t> ap;
  std::vector<uint32_t> fl, lb;
  std::vector<uint16_t> tn;
  int rc;
  if ((rc = pull(ac, c.alloc_cpu, 1)) || (rc = pull(am, c.alloc_mem, 1)) || (rc = pull(ae, c.alloc_eph, 1)) ||
      (rc = pull(as, c.alloc_scalar, (size_t)c.n_scalar)) || (rc = pull(ap, c.alloc_pods, 1)) ||
      (rc = pull(fl, c.flags, 1)) || (rc = pull(tn, c.taints, KSIM_MAX_NODE_TAINTS)) ||
      (rc = pull(lb, c.labels, (size_t)c.n_label_cols)) || (rc = pull(nbl, c.nb_limit, 1)))
    return rc;
  // the dynamic columns as last uploaded (the replay adds the binds since), into the table
  ksim_node_table t{};
  std::vector<std::vector<char>> snaps;   // moving a vector keeps its buffer: the table's pointers stay good
  rc = for_dyn_cols(h, nullptr, [&](auto col) -> int {
    using T = typename decltype(col)::value_type;
    std::vector<T> out;
    if (const int r = pull(out, col.snap, (size_t)col.rows)) return r;
    const char* bytes = (const char*)out.data();
    snaps.emplace_back(bytes, bytes + sizeof(T) * out.size());
    t.*col.field = (const T*)snaps.back().data();
    return KSIM_OK;
  });
  if (rc) return rc;
  std::vector<uint8_t> te(h->taint_effect);
  std::vector<int32_t> lco((size_t)c.n_label_cols);
  std::vector<int64_t> lnum((size_t)std::max(c.n_label_values, 0));
  std::vector<uint8_t> lok((size_t)std::max(c.n_label_values, 0));
  std::vector<double> tlog((size_t)c.n_topo_log);
  if (!lco.empty()) HIPCHK(h, hcopy(h, lco.data(), c.label_col_offset, 4 * lco.size(), hipMemcpyDeviceToHost));
  if (!lnum.empty()) {
    HIPCHK(h, hcopy(h, lnum.data(), c.label_num, 8 * lnum.size(), hipMemcpyDeviceToHost));
    HIPCHK(h, hcopy(h, lok.data(), c.label_num_ok, lok.size(), hipMemcpyDeviceToHost));
  }
  if (!tlog.empty()) HIPCHK(h, hcopy(h, tlog.data(), c.topo_log, 8 * tlog.size(), hipMemcpyDeviceToHost));
  t.n_nodes = n;
  t.n_scalar = c.n_scalar;
  t.n_label_cols = c.n_label_cols;
  t.alloc_cpu = ac.data();
  t.alloc_mem = am.data();
  t.alloc_eph = ae.data();
  t.alloc_pods = ap.data();
  t.alloc_scalar = as.data();
  t.flags = fl.data();
  t.taints = tn.data();
  t.labels = lb.data();
  t.n_classes = c.n_classes;
  t.nb_limit = nbl.data();
  ksim_vocab v{};
  v.n_taints = (int32_t)te.size();
  v.n_label_values = c.n_label_values;
  v.taint_effect = te.data();
  v.label_col_offset = lco.data();
  v.label_num = lnum.data();
  v.label_num_ok = lok.data();
  v.n_topo_log = c.n_topo_log;
  v.topo_log = tlog.data();
  std::vector<int32_t> old_pos((size_t)std::max(n, 1));
  for (int32_t i = 0; i < n; i++) old_pos[i] = i < pos ? i : i + 1;
  return ksim_upsert_nodes(h, &t, &v, old_pos.data());
}

int ksim_get_node_state(ksim_handle* h, int64_t* req_cpu, int64_t* req_mem, int64_t* req_eph, int64_t* nz_cpu,
                        int64_t* nz_mem, int32_t* num_pods) {
  if (!h || !h->has_cluster) return set_err(h, KSIM_E_INVALID, "cluster not set");
  if (int rc = flush_idle(h)) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  const size_t N = (size_t)h->dc.n;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (req_cpu) HIPCHK(h, hcopy(h, req_cpu, h->dc.req_cpu, 8 * N, hipMemcpyDeviceToHost));
  if (req_mem) HIPCHK(h, hcopy(h, req_mem, h->dc.req_mem, 8 * N, hipMemcpyDeviceToHost));
  if (req_eph) HIPCHK(h, hcopy(h, req_eph, h->dc.req_eph, 8 * N, hipMemcpyDeviceToHost));
  if (nz_cpu) HIPCHK(h, hcopy(h, nz_cpu, h->dc.nz_cpu, 8 * N, hipMemcpyDeviceToHost));
  if (nz_mem) HIPCHK(h, hcopy(h, nz_mem, h->dc.nz_mem, 8 * N, hipMemcpyDeviceToHost));
  if (num_pods) HIPCHK(h, hcopy(h, num_pods, h->dc.num_pods, 4 * N, hipMemcpyDeviceToHost));
  return KSIM_OK;
}

int ksim_get_nb_alloc(ksim_handle* h, int64_t* out) {
  if (!h || !h->has_cluster || !out) return set_err(h, KSIM_E_INVALID, "cluster not set / null out");
  if (int rc = flush_idle(h)) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hcopy(h, out, h->dc.nb_alloc, 8 * (size_t)h->dc.n, hipMemcpyDeviceToHost));
  return KSIM_OK;
}

int ksim_set_volume_limits(ksim_handle* h, int32_t n_families, const int32_t* family_plugin, const int32_t* limit,
                           const int32_t* attached) {
  if (const int prc = flush_pend_bind(h)) return prc;   // a queued Reserve lands first
  if (!h || !h->has_cluster) return set_err(h, KSIM_E_INVALID, "ksim_set_volume_limits before ksim_set_cluster");
  if (is_sharded(h) || h->replicated || h->world > 1)
    return set_err(h, KSIM_E_UNSUPPORTED, "ksim_set_volume_limits on a shard or replicated handle");
  if (n_families < 0 || n_families > KSIM_MAX_VOL_FAMILIES)
    return set_err(h, KSIM_E_INVALID, "n_families out of range");
  const size_t N = (size_t)h->dc.n;
  if (n_families > 0 && (!family_plugin || (N > 0 && (!limit || !attached))))
    return set_err(h, KSIM_E_INVALID, "null volume table");
  uint32_t plug = 0;
  for (int32_t f = 0; f < n_families; f++) {
    if (family_plugin[f] < KSIM_PL_EBS_LIMITS || family_plugin[f] > KSIM_PL_AZURE_DISK_LIMITS)
      return set_err(h, KSIM_E_INVALID, "family_plugin is not a volume limit plugin");
    plug |= (uint32_t)(family_plugin[f] - KSIM_PL_EBS_LIMITS) << (4 * f);
  }
  for (size_t i = 0; i < N * (size_t)n_families; i++)
    if (limit[i] < 0 || attached[i] < 0) return set_err(h, KSIM_E_INVALID, "negative volume limit / attached count");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  // the kernels take the cluster by value, and a pod's validation and plan
  // depend on the table: captured graphs and the loaded queue go
  drop_graphs(h);
  h->dp = DevPods{};
  h->batchable.clear();
  h->vol_bufs.clear();
  h->bound.vol = BoundList{};           // the bound pods' holdings named the old table's families
  h->bound.voff = nullptr;
  h->bound.vols = nullptr;
  h->bound.alt.voff2 = nullptr;           // (ksim_preempt_commit's second set of them went with the buffers)
  h->bound.alt.vols2 = nullptr;
  h->vol_init = nullptr;
  h->dc.vol_nf = 0;
  h->dc.vol_plug = 0;
  h->dc.vol_limit = nullptr;
  h->dc.vol_attached = nullptr;
  if (n_families == 0) return KSIM_OK;
  const size_t bytes = 4 * N * (size_t)n_families;
  const int32_t* dl = nullptr;
  int32_t *da = nullptr, *di = nullptr;
  int rc;
  if ((rc = h->vol_bufs.alloc(h, dl, bytes, limit)) || (rc = h->vol_bufs.alloc(h, da, bytes, attached)) ||
      (rc = h->vol_bufs.alloc(h, di, bytes, attached))) {
    h->vol_bufs.clear();
    return rc;
  }
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->dc.vol_nf = n_families;
  h->dc.vol_plug = plug;
  h->dc.vol_limit = dl;
  h->dc.vol_attached = da;
  h->vol_init = di;
  return KSIM_OK;
}

int ksim_get_volume_attached(ksim_handle* h, int32_t* out) {
  if (!h || !h->has_cluster || !out) return set_err(h, KSIM_E_INVALID, "cluster not set / null out");
  if (!h->dc.vol_nf) return set_err(h, KSIM_E_INVALID, "no volume table (ksim_set_volume_limits)");
  if (int rc = flush_idle(h)) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hcopy(h, out, h->dc.vol_attached, 4 * (size_t)h->dc.n * h->dc.vol_nf, hipMemcpyDeviceToHost));
  return KSIM_OK;
}

int ksim_get_class_count(ksim_handle* h, int32_t* out) {
  if (!h || !h->has_cluster || !out) return set_err(h, KSIM_E_INVALID, "cluster not set / null out");
  if (int rc = flush_idle(h)) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (h->dc.n_classes)
    HIPCHK(h, hcopy(h, out, h->dc.cnt, 4 * (size_t)h->dc.n * h->dc.n_classes, hipMemcpyDeviceToHost));
  return KSIM_OK;
}

int ksim_get_next_start(ksim_handle* h, int32_t* next_start) {
  if (const int prc = flush_pend_bind(h)) return prc;   // a queued Reserve lands first
  if (!h || !next_start) return KSIM_E_INVALID;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hcopy(h, next_start, &h->st->next_start, 4, hipMemcpyDeviceToHost));
  return KSIM_OK;
}

int ksim_set_next_start(ksim_handle* h, int32_t next_start) {
  if (const int prc = flush_pend_bind(h)) return prc;   // a queued Reserve lands first
  if (!h) return KSIM_E_INVALID;
  // a global position: a node shard scans the whole ring (dc.n_total == dc.n unsharded)
  if (h->has_cluster && (next_start < 0 || next_start >= std::max(h->dc.n_total, 1)))
    return set_err(h, KSIM_E_INVALID, "next_start out of range");
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hcopy(h, &h->st->next_start, &next_start, 4, hipMemcpyHostToDevice));
  return KSIM_OK;
}

int ksim_set_pod_seq(ksim_handle* h, int64_t seq) {
  if (const int prc = flush_pend_bind(h)) return prc;   // a queued Reserve lands first
  if (!h) return KSIM_E_INVALID;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hcopy(h, &h->st->pod_seq, &seq, 8, hipMemcpyHostToDevice));
  return KSIM_OK;
}

int ksim_reset_cluster(ksim_handle* h) {
  if (const int prc = flush_pend_bind(h)) return prc;   // a queued Reserve lands first
  if (!h || !h->has_cluster) return set_err(h, KSIM_E_INVALID, "cluster not set");
  // the static table stays: k_static_table reads a node's flags, taints and
  // labels (static_filters_pass, count_intolerable_prefer, pref_term_mask),
  // none of the columns restored here
  HIPCHK(h, hipSetDevice(h->device));
  const size_t N = (size_t)h->dc.n;
  // the dynamic columns from their snapshot copies and the run state zeroed,
  // in one launch (every buffer is a hipMalloc allocation: 16-byte aligned)
  ResetList L;
  hipError_t fe = hipSuccess;
  auto put = [&](void* d, const void* s, size_t bytes) {   // an entry the launch cannot take: its own copy
    if (L.add(d, s, bytes) || fe != hipSuccess) return;
    fe = s ? hipMemcpyAsync(d, s, bytes, hipMemcpyDeviceToDevice, h->stream) : hipMemsetAsync(d, 0, bytes, h->stream);
  };
  (void)for_dyn_cols(h, nullptr, [&](auto col) -> int {   // a column without rows (no scalars, no classes) has no entry
    if (col.rows) put(col.live, col.snap, sizeof(*col.live) * N * (size_t)col.rows);
    return KSIM_OK;
  });
  static_assert(sizeof(DevState) % 4 == 0, "DevState by words");
  put(h->st, nullptr, sizeof(DevState));
  HIPCHK(h, fe);
  if (L.n) launch_reset_copy(L, h->stream);
  launch_ptab_init(h->dc, h->dp, h->stream);        // the queue's persistent tables follow the counts
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return KSIM_OK;
}
