/* bng_ext.cpp — torch extension binding for the CDNA4 BNG dataplane.
 *
 * The Python-visible surface of the HIP dataplane: takes torch tensors
 * (device table blobs + packet batches), validates shape/device, and
 * launches the kernels on the current HIP stream so every table mutation
 * is stream-ordered with packet processing (BPF-map consistency).
 *
 * Also exports the struct layout report that tests/test_abi.py checks
 * against the Python ctypes mirrors (the analog of the reference's
 * test/ebpf/maps_test.go struct-ABI tests).
 */
#include <torch/extension.h>
#include <climits>
#include <hip/hip_runtime.h>
#include <c10/hip/HIPStream.h>

#include "bng_abi.h"
#include "bng_params.h"
#include "bng_launch.h"

namespace {

hipStream_t cur_stream() {
  return c10::hip::getCurrentHIPStream().stream();
}

hipStream_t g_svc_stream = nullptr;   /* persistent-service stream */

/* CU partitioning (the saturated-tail lever): reserve the first
 * `svc_cus` CUs for the resident service and launch the batched
 * pipeline on the complementary mask, so a 100% data flood cannot
 * co-schedule on the service CUs.  Costs the pipeline svc_cus/256 of
 * its capacity. */
hipStream_t g_masked_stream = nullptr;
int g_svc_cus = 0;

void set_cu_partition(int64_t svc_cus) {
  TORCH_CHECK(svc_cus >= 0 && svc_cus <= 64, "svc_cus in [0,64]");
  TORCH_CHECK(g_svc_stream == nullptr && g_masked_stream == nullptr,
              "set_cu_partition must run before the first service "
              "start / masked launch");
  g_svc_cus = (int)svc_cus;
}

hipStream_t masked_stream() {
  if (!g_masked_stream) {
    if (g_svc_cus > 0) {
      /* reserved CUs are spread one per 32-CU mask word so BOTH
       * partitions keep CUs in every XCD/SE (a mask concentrated in
       * word0 hung the masked stream on hardware) */
      uint32_t mask[8];
      for (int i = 0; i < 8; ++i) mask[i] = 0xFFFFFFFFu;
      for (int c = 0; c < g_svc_cus; ++c)
        mask[c % 8] &= ~(1u << (c / 8));
      (void)hipExtStreamCreateWithCUMask(&g_masked_stream, 8, mask);
    } else {
      (void)hipStreamCreateWithFlags(&g_masked_stream,
                                     hipStreamNonBlocking);
    }
  }
  return g_masked_stream;
}

void masked_sync() {
  if (g_masked_stream) (void)hipStreamSynchronize(g_masked_stream);
}

/* Fences that make a masked launch transparent to the caller's stream
 * order: the masked stream waits for prior work on the current stream,
 * and the current stream waits for the masked kernel — so bench's
 * event machinery (prep/work_free) keeps working unchanged. */
hipEvent_t g_fence_pre = nullptr, g_fence_post = nullptr;

hipStream_t masked_entry(hipStream_t cur) {
  hipStream_t st = masked_stream();
  if (!g_fence_pre) {
    (void)hipEventCreateWithFlags(&g_fence_pre, hipEventDisableTiming);
    (void)hipEventCreateWithFlags(&g_fence_post, hipEventDisableTiming);
  }
  (void)hipEventRecord(g_fence_pre, cur);
  (void)hipStreamWaitEvent(st, g_fence_pre, 0);
  return st;
}

void masked_exit(hipStream_t st, hipStream_t cur) {
  (void)hipEventRecord(g_fence_post, st);
  (void)hipStreamWaitEvent(cur, g_fence_post, 0);
}

void check_dev(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be a device tensor");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}

uint32_t table_mask(const torch::Tensor& t, size_t entry, const char* name) {
  size_t n = (size_t)t.numel() * t.element_size() / entry;
  TORCH_CHECK(n > 0 && (n & (n - 1)) == 0, name,
              " slot count must be a power of two, got ", n);
  return (uint32_t)(n - 1);
}

void dhcp_fastpath(torch::Tensor data, torch::Tensor in_len,
                   torch::Tensor out_len, torch::Tensor verdict,
                   torch::Tensor subs, torch::Tensor pools,
                   torch::Tensor cfg, torch::Tensor stats, int64_t now_sec,
                   c10::optional<torch::Tensor> now_buf) {
  check_dev(data, "data"); check_dev(subs, "subs");
  int n = in_len.numel();
  int stride = data.size(1);
  bng_launch_dhcp(data.data_ptr(), in_len.data_ptr(), out_len.data_ptr(),
                  verdict.data_ptr(), n, stride, subs.data_ptr(),
                  table_mask(subs, sizeof(bng_sub_entry), "subs"),
                  pools.data_ptr(),
                  (uint32_t)(pools.numel() * pools.element_size() /
                             sizeof(bng_ip_pool)),
                  cfg.data_ptr(), stats.data_ptr(), (uint64_t)now_sec,
                  now_buf.has_value() ? now_buf->data_ptr() : nullptr,
                  cur_stream());
}

void nat44(torch::Tensor data, torch::Tensor in_len, torch::Tensor verdict,
           bool is_egress, torch::Tensor sessions, torch::Tensor reverse,
           torch::Tensor eim, torch::Tensor subnat, torch::Tensor cfg,
           torch::Tensor hairpin, int64_t n_hairpin, torch::Tensor stats,
           torch::Tensor log_ring, torch::Tensor log_hdr, int64_t now_ns) {
  check_dev(data, "data"); check_dev(sessions, "sessions");
  int n = in_len.numel();
  int stride = data.size(1);
  bng_launch_nat44(
      data.data_ptr(), in_len.data_ptr(), verdict.data_ptr(), n, stride,
      is_egress ? 1 : 0, sessions.data_ptr(),
      table_mask(sessions, sizeof(bng_nat_session), "sessions"),
      reverse.data_ptr(), table_mask(reverse, sizeof(bng_nat_reverse), "reverse"),
      eim.data_ptr(), table_mask(eim, sizeof(bng_eim_entry), "eim"),
      subnat.data_ptr(), table_mask(subnat, sizeof(bng_subctx), "subctx"),
      cfg.data_ptr(), hairpin.data_ptr(), (uint32_t)n_hairpin,
      stats.data_ptr(), log_ring.data_ptr(), log_hdr.data_ptr(),
      (uint64_t)now_ns, cur_stream());
}

void qos(torch::Tensor data, torch::Tensor in_len, torch::Tensor verdict,
         bool is_egress, torch::Tensor table, torch::Tensor stats,
         int64_t now_ns) {
  check_dev(data, "data"); check_dev(table, "table");
  bng_launch_qos(data.data_ptr(), in_len.data_ptr(), verdict.data_ptr(),
                 (int)in_len.numel(), (int)data.size(1), is_egress ? 1 : 0,
                 table.data_ptr(),
                 /* bng_qos_bucket (egress) and bng_subctx (ingress) are
                    both 64 B, so one mask computation serves both */
                 table_mask(table, sizeof(bng_qos_bucket), "qos"),
                 stats.data_ptr(), (uint64_t)now_ns, cur_stream());
}

void antispoof(torch::Tensor data, torch::Tensor in_len,
               torch::Tensor verdict, torch::Tensor bindings,
               torch::Tensor cfg, torch::Tensor stats, torch::Tensor ring,
               torch::Tensor hdr, int64_t now_ns) {
  check_dev(data, "data"); check_dev(bindings, "bindings");
  bng_launch_antispoof(
      data.data_ptr(), in_len.data_ptr(), verdict.data_ptr(),
      (int)in_len.numel(), (int)data.size(1), bindings.data_ptr(),
      table_mask(bindings, sizeof(bng_binding_entry), "bindings"),
      cfg.data_ptr(), stats.data_ptr(), ring.data_ptr(), hdr.data_ptr(),
      (uint64_t)now_ns, cur_stream());
}

void uplink_pipeline(torch::Tensor data, torch::Tensor in_len,
                     torch::Tensor out_len, torch::Tensor verdict,
                     torch::Tensor subs, torch::Tensor pools,
                     torch::Tensor scfg, torch::Tensor dhcp_stats,
                     torch::Tensor bindings, torch::Tensor acfg,
                     torch::Tensor as_stats, torch::Tensor spoof_ring,
                     torch::Tensor spoof_hdr, torch::Tensor sessions,
                     torch::Tensor reverse, torch::Tensor eim,
                     torch::Tensor subctx, torch::Tensor ncfg,
                     torch::Tensor hairpin, int64_t n_hairpin,
                     torch::Tensor nat_stats, torch::Tensor log_ring,
                     torch::Tensor log_hdr, torch::Tensor qos_eg,
                     torch::Tensor qos_stats, int64_t now_ns,
                     int64_t now_sec,
                     c10::optional<torch::Tensor> order,
                     bool downlink,
                     c10::optional<torch::Tensor> now_buf,
                     bool masked) {
  check_dev(data, "data");
  bng_uplink_params P{};
  P.now_ptr = now_buf.has_value()
      ? (const uint64_t*)now_buf->data_ptr() : nullptr;
  P.data = (uint8_t*)data.data_ptr();
  P.in_len = (const uint16_t*)in_len.data_ptr();
  P.out_len = (uint16_t*)out_len.data_ptr();
  P.verdict = (uint8_t*)verdict.data_ptr();
  P.order = order.has_value() ? (const int32_t*)order->data_ptr() : nullptr;
  P.n = (int)in_len.numel();
  P.stride = (int)data.size(1);
  P.subs = (const bng_sub_entry*)subs.data_ptr();
  P.sub_mask = table_mask(subs, sizeof(bng_sub_entry), "subs");
  P.pools = (const bng_ip_pool*)pools.data_ptr();
  P.n_pools = (uint32_t)(pools.numel() * pools.element_size() /
                         sizeof(bng_ip_pool));
  P.scfg = (const bng_server_config*)scfg.data_ptr();
  P.dhcp_stats = (unsigned long long*)dhcp_stats.data_ptr();
  P.bindings = (const bng_binding_entry*)bindings.data_ptr();
  P.bmask = table_mask(bindings, sizeof(bng_binding_entry), "bindings");
  P.acfg = (const bng_antispoof_config*)acfg.data_ptr();
  P.as_stats = (unsigned long long*)as_stats.data_ptr();
  P.spoof_ring = (bng_spoof_event*)spoof_ring.data_ptr();
  P.spoof_hdr = (bng_ring_header*)spoof_hdr.data_ptr();
  P.sessions = (bng_nat_session*)sessions.data_ptr();
  P.sess_mask = table_mask(sessions, sizeof(bng_nat_session), "sessions");
  P.reverse = (bng_nat_reverse*)reverse.data_ptr();
  P.rev_mask = table_mask(reverse, sizeof(bng_nat_reverse), "reverse");
  P.eim = (bng_eim_entry*)eim.data_ptr();
  P.eim_mask = table_mask(eim, sizeof(bng_eim_entry), "eim");
  P.subctx = (bng_subctx*)subctx.data_ptr();
  P.subctx_mask = table_mask(subctx, sizeof(bng_subctx), "subctx");
  P.ncfg = (const bng_nat_config*)ncfg.data_ptr();
  P.hairpin_ips = (const uint32_t*)hairpin.data_ptr();
  P.n_hairpin = (uint32_t)n_hairpin;
  P.nat_stats = (unsigned long long*)nat_stats.data_ptr();
  P.log_ring = (bng_nat_log_entry*)log_ring.data_ptr();
  P.log_hdr = (bng_ring_header*)log_hdr.data_ptr();
  P.qos_eg = (bng_qos_bucket*)qos_eg.data_ptr();
  P.qos_eg_mask = table_mask(qos_eg, sizeof(bng_qos_bucket), "qos");
  P.qos_stats = (unsigned long long*)qos_stats.data_ptr();
  P.now_ns = (uint64_t)now_ns;
  P.now_sec = (uint64_t)now_sec;
  hipStream_t cur = cur_stream();
  hipStream_t st = masked ? masked_entry(cur) : cur;
  if (downlink)
    bng_launch_downlink(&P, st);
  else
    bng_launch_uplink(&P, st);
  if (masked) masked_exit(st, cur);
}

void pkt_class(torch::Tensor data, torch::Tensor in_len,
               torch::Tensor cls) {
  bng_launch_pkt_class(data.data_ptr(), in_len.data_ptr(), cls.data_ptr(),
                       (int)in_len.numel(), (int)data.size(1),
                       cur_stream());
}

/* Table-management entry points.  The kernels index the batch and rc by
 * thread id and the table by (hash & mask), so every size is checked here:
 * a short rc would be an out-of-bounds device write. */
size_t nbytes(const torch::Tensor& t) {
  return (size_t)t.numel() * t.element_size();
}

uint32_t dev_table_mask(const torch::Tensor& t, size_t entry,
                        const char* name) {
  check_dev(t, name);
  return table_mask(t, entry, name);
}

/* Checks an upsert's batch and rc; returns the record count (0 = nothing
 * to launch). */
int upsert_count(const torch::Tensor& batch, size_t entry,
                 const torch::Tensor& rc) {
  check_dev(batch, "batch"); check_dev(rc, "rc");
  TORCH_CHECK(nbytes(batch) % entry == 0, "batch must be a whole number of ",
              entry, "-byte entries, got ", nbytes(batch), " bytes");
  size_t n = nbytes(batch) / entry;
  TORCH_CHECK(n <= (size_t)INT_MAX, "batch too large");
  TORCH_CHECK(rc.element_size() == 4 && (size_t)rc.numel() >= n,
              "rc must hold one int32 per record");
  return (int)n;
}

/* Checks a delete's keys; returns the key count. */
int delete_count(const torch::Tensor& keys) {
  check_dev(keys, "keys");
  TORCH_CHECK(keys.element_size() == 8, "keys must be 64-bit");
  TORCH_CHECK(keys.numel() <= INT_MAX, "too many keys");
  return (int)keys.numel();
}

void sub_upsert(torch::Tensor table, torch::Tensor batch, torch::Tensor rc) {
  uint32_t mask = dev_table_mask(table, sizeof(bng_sub_entry), "subs");
  int n = upsert_count(batch, sizeof(bng_sub_entry), rc);
  if (n == 0) return;
  bng_launch_sub_upsert(table.data_ptr(), mask, batch.data_ptr(), n,
                        rc.data_ptr(), cur_stream());
}
void sess_import(torch::Tensor sessions, torch::Tensor reverse,
                 torch::Tensor eim, torch::Tensor batch, torch::Tensor rc) {
  uint32_t sess_mask = dev_table_mask(sessions, sizeof(bng_nat_session),
                                      "sessions");
  uint32_t rev_mask = dev_table_mask(reverse, sizeof(bng_nat_reverse),
                                     "reverse");
  uint32_t eim_mask = dev_table_mask(eim, sizeof(bng_eim_entry), "eim");
  int n = upsert_count(batch, sizeof(bng_sess_export), rc);
  if (n == 0) return;
  bng_launch_sess_import(sessions.data_ptr(), sess_mask, reverse.data_ptr(),
                         rev_mask, eim.data_ptr(), eim_mask,
                         batch.data_ptr(), n, rc.data_ptr(), cur_stream());
}
void sub_delete(torch::Tensor table, torch::Tensor keys) {
  uint32_t mask = dev_table_mask(table, sizeof(bng_sub_entry), "subs");
  int n = delete_count(keys);
  if (n == 0) return;
  bng_launch_sub_delete(table.data_ptr(), mask, keys.data_ptr(), n,
                        cur_stream());
}
void subctx_upsert(torch::Tensor table, torch::Tensor batch,
                   int64_t update_mask, torch::Tensor rc) {
  uint32_t mask = dev_table_mask(table, sizeof(bng_subctx), "subctx");
  int n = upsert_count(batch, sizeof(bng_subctx), rc);
  if (n == 0) return;
  bng_launch_subctx_upsert(table.data_ptr(), mask, batch.data_ptr(), n,
                           (uint32_t)update_mask, rc.data_ptr(),
                           cur_stream());
}
void qos_upsert(torch::Tensor table, torch::Tensor batch, torch::Tensor rc) {
  uint32_t mask = dev_table_mask(table, sizeof(bng_qos_bucket), "qos");
  int n = upsert_count(batch, sizeof(bng_qos_bucket), rc);
  if (n == 0) return;
  bng_launch_qos_upsert(table.data_ptr(), mask, batch.data_ptr(), n,
                        rc.data_ptr(), cur_stream());
}
void binding_upsert(torch::Tensor table, torch::Tensor batch,
                    torch::Tensor rc) {
  uint32_t mask = dev_table_mask(table, sizeof(bng_binding_entry), "bindings");
  int n = upsert_count(batch, sizeof(bng_binding_entry), rc);
  if (n == 0) return;
  bng_launch_binding_upsert(table.data_ptr(), mask, batch.data_ptr(), n,
                            rc.data_ptr(), cur_stream());
}
void binding_delete(torch::Tensor table, torch::Tensor keys) {
  uint32_t mask = dev_table_mask(table, sizeof(bng_binding_entry), "bindings");
  int n = delete_count(keys);
  if (n == 0) return;
  bng_launch_binding_delete(table.data_ptr(), mask, keys.data_ptr(), n,
                            cur_stream());
}

void nat_sweep(torch::Tensor sessions, torch::Tensor reverse,
               torch::Tensor subnat, torch::Tensor eim, int64_t eim_to,
               int64_t now_ns, int64_t udp_to,
               int64_t tcp_est_to, int64_t tcp_tr_to, int64_t icmp_to,
               torch::Tensor stats) {
  check_dev(sessions, "sessions"); check_dev(eim, "eim");
  check_dev(stats, "stats");
  uint32_t n_slots = (uint32_t)(nbytes(sessions) / sizeof(bng_nat_session));
  uint32_t eim_slots = (uint32_t)(nbytes(eim) / sizeof(bng_eim_entry));
  bng_launch_nat_sweep(
      sessions.data_ptr(), n_slots, reverse.data_ptr(),
      dev_table_mask(reverse, sizeof(bng_nat_reverse), "reverse"),
      subnat.data_ptr(), dev_table_mask(subnat, sizeof(bng_subctx), "subctx"),
      eim.data_ptr(), eim_slots, (uint64_t)eim_to,
      (uint64_t)now_ns, (uint64_t)udp_to, (uint64_t)tcp_est_to,
      (uint64_t)tcp_tr_to, (uint64_t)icmp_to, stats.data_ptr(),
      cur_stream());
}

void shard_owner(torch::Tensor data, torch::Tensor in_len,
                 torch::Tensor owner, int64_t n_shards) {
  bng_launch_shard_owner(data.data_ptr(), in_len.data_ptr(),
                         owner.data_ptr(), (int)in_len.numel(),
                         (int)data.size(1), (int)n_shards, cur_stream());
}

/* PPPoE session-data fast path.  Both packet kernels move 16-B words
 * inside a row, so the batch must be 16-B aligned with a stride that is a
 * multiple of 16 (every batch the launcher and the pump build is). */
void check_pppoe_batch(const torch::Tensor& data, const torch::Tensor& in_len,
                       const torch::Tensor& sess) {
  check_dev(data, "data"); check_dev(in_len, "in_len");
  check_dev(sess, "pppoe_sess");
  TORCH_CHECK(data.dim() == 2 && data.element_size() == 1,
              "data must be [n, stride] bytes");
  TORCH_CHECK(data.size(0) == in_len.numel() && in_len.element_size() == 2,
              "in_len must hold one 16-bit length per row");
  TORCH_CHECK(data.size(1) >= 64 && data.size(1) % 16 == 0 &&
              data.size(1) <= 65535,
              "PPPoE fast path needs a stride that is a multiple of 16, "
              "64..65535");
  TORCH_CHECK(((uintptr_t)data.data_ptr() & 15) == 0,
              "PPPoE fast path needs a 16-byte aligned batch");
  TORCH_CHECK((size_t)sess.numel() * sess.element_size() ==
              (size_t)BNG_PPPOE_MAX_SESSIONS * sizeof(bng_pppoe_sess),
              "pppoe_sess must hold 65536 entries");
}

void pppoe_decap(torch::Tensor data, torch::Tensor in_len,
                 torch::Tensor state, torch::Tensor sess,
                 torch::Tensor stats) {
  check_pppoe_batch(data, in_len, sess);
  check_dev(state, "state"); check_dev(stats, "stats");
  TORCH_CHECK(state.numel() == in_len.numel() && state.element_size() == 1,
              "state must hold one byte per row");
  TORCH_CHECK(stats.numel() * stats.element_size() >=
              (long)(BNG_PPPOE_NSTATS * sizeof(uint64_t)), "stats too small");
  int n = (int)in_len.numel();
  if (n == 0) return;
  bng_launch_pppoe_decap(data.data_ptr(), in_len.data_ptr(),
                         state.data_ptr(), n, (int)data.size(1),
                         sess.data_ptr(), stats.data_ptr(), cur_stream());
}

void pppoe_encap(torch::Tensor data, torch::Tensor in_len,
                 torch::Tensor verdict, torch::Tensor state,
                 torch::Tensor by_ip, torch::Tensor sess,
                 torch::Tensor scfg, torch::Tensor stats) {
  check_pppoe_batch(data, in_len, sess);
  check_dev(verdict, "verdict"); check_dev(state, "state");
  check_dev(by_ip, "pppoe_by_ip"); check_dev(scfg, "scfg");
  check_dev(stats, "stats");
  TORCH_CHECK(state.numel() == in_len.numel() && state.element_size() == 1 &&
              verdict.numel() == in_len.numel() &&
              verdict.element_size() == 1,
              "verdict and state must hold one byte per row");
  TORCH_CHECK(stats.numel() * stats.element_size() >=
              (long)(BNG_PPPOE_NSTATS * sizeof(uint64_t)), "stats too small");
  TORCH_CHECK(scfg.numel() * scfg.element_size() >=
              (long)sizeof(bng_server_config), "scfg too small");
  int n = (int)in_len.numel();
  if (n == 0) return;
  bng_launch_pppoe_encap(
      data.data_ptr(), in_len.data_ptr(), verdict.data_ptr(),
      state.data_ptr(), n, (int)data.size(1), by_ip.data_ptr(),
      table_mask(by_ip, sizeof(bng_pppoe_ip), "pppoe_by_ip"),
      sess.data_ptr(), scfg.data_ptr(), stats.data_ptr(), cur_stream());
}

void pppoe_sess_upsert(torch::Tensor sess, torch::Tensor by_ip,
                       torch::Tensor batch, torch::Tensor rc) {
  check_dev(sess, "pppoe_sess");
  TORCH_CHECK(nbytes(sess) ==
              (size_t)BNG_PPPOE_MAX_SESSIONS * sizeof(bng_pppoe_sess),
              "pppoe_sess must hold 65536 entries");
  uint32_t mask = dev_table_mask(by_ip, sizeof(bng_pppoe_ip), "pppoe_by_ip");
  int n = upsert_count(batch, sizeof(bng_pppoe_sess), rc);
  if (n == 0) return;
  bng_launch_pppoe_sess_upsert(sess.data_ptr(), by_ip.data_ptr(), mask,
                               batch.data_ptr(), n, rc.data_ptr(),
                               cur_stream());
}

void pppoe_sess_delete(torch::Tensor sess, torch::Tensor by_ip,
                       torch::Tensor sids) {
  check_dev(sess, "pppoe_sess"); check_dev(by_ip, "pppoe_by_ip");
  check_dev(sids, "sids");
  TORCH_CHECK((size_t)sess.numel() * sess.element_size() ==
              (size_t)BNG_PPPOE_MAX_SESSIONS * sizeof(bng_pppoe_sess),
              "pppoe_sess must hold 65536 entries");
  TORCH_CHECK(sids.element_size() == 4, "sids must be int32");
  int n = (int)sids.numel();
  if (n == 0) return;
  bng_launch_pppoe_sess_delete(
      sess.data_ptr(), by_ip.data_ptr(),
      table_mask(by_ip, sizeof(bng_pppoe_ip), "pppoe_by_ip"),
      sids.data_ptr(), n, cur_stream());
}

/* Per-subscriber traffic accounting.  The packet kernels read rows with
 * 16-B loads up to byte 47, the commit indexes slot / verdict / out_len by
 * packet id and the table by slot, so every size is checked here. */
uint32_t acct_table_mask(const torch::Tensor& table) {
  return dev_table_mask(table, sizeof(bng_acct_entry), "acct");
}

void check_acct_batch(const torch::Tensor& data,
                      const torch::Tensor& in_len) {
  check_dev(data, "data"); check_dev(in_len, "in_len");
  TORCH_CHECK(data.dim() == 2 && data.element_size() == 1,
              "data must be [n, stride] bytes");
  TORCH_CHECK(data.size(0) == in_len.numel() && in_len.element_size() == 2,
              "in_len must hold one 16-bit length per row");
  TORCH_CHECK(data.size(1) >= 64 && data.size(1) % 16 == 0 &&
              data.size(1) <= 65535,
              "accounting needs a stride that is a multiple of 16, "
              "64..65535");
  TORCH_CHECK(((uintptr_t)data.data_ptr() & 15) == 0,
              "accounting needs a 16-byte aligned batch");
}

void acct_resolve(torch::Tensor data, torch::Tensor in_len,
                  torch::Tensor slot, torch::Tensor table) {
  check_acct_batch(data, in_len);
  check_dev(slot, "slot");
  TORCH_CHECK(slot.element_size() == 4 && slot.numel() >= in_len.numel(),
              "slot must hold one int32 per row");
  uint32_t mask = acct_table_mask(table);
  int n = (int)in_len.numel();
  if (n == 0) return;
  bng_launch_acct_resolve(data.data_ptr(), in_len.data_ptr(),
                          slot.data_ptr(), n, (int)data.size(1),
                          table.data_ptr(), mask, cur_stream());
}

void acct_commit(torch::Tensor table, torch::Tensor slot,
                 torch::Tensor verdict, torch::Tensor out_len,
                 int64_t now_ns) {
  check_dev(slot, "slot"); check_dev(verdict, "verdict");
  check_dev(out_len, "out_len");
  int64_t n = verdict.numel();
  TORCH_CHECK(n <= INT_MAX, "batch too large");
  TORCH_CHECK(verdict.element_size() == 1, "verdict must be bytes");
  TORCH_CHECK(slot.element_size() == 4 && slot.numel() >= n,
              "slot must hold one int32 per row");
  TORCH_CHECK(out_len.element_size() == 2 && out_len.numel() == n,
              "out_len must hold one 16-bit length per row");
  uint32_t mask = acct_table_mask(table);
  if (n == 0) return;
  bng_launch_acct_commit(table.data_ptr(), mask, slot.data_ptr(),
                         verdict.data_ptr(), out_len.data_ptr(), (int)n,
                         (uint64_t)now_ns, cur_stream());
}

void acct_downlink(torch::Tensor data, torch::Tensor in_len,
                   torch::Tensor verdict, torch::Tensor table,
                   int64_t now_ns) {
  check_acct_batch(data, in_len);
  check_dev(verdict, "verdict");
  TORCH_CHECK(verdict.numel() == in_len.numel() &&
              verdict.element_size() == 1,
              "verdict must hold one byte per row");
  uint32_t mask = acct_table_mask(table);
  int n = (int)in_len.numel();
  if (n == 0) return;
  bng_launch_acct_downlink(data.data_ptr(), in_len.data_ptr(),
                           verdict.data_ptr(), n, (int)data.size(1),
                           table.data_ptr(), mask, (uint64_t)now_ns,
                           cur_stream());
}

/* Checks the address list of an accounting CRUD call; returns its count. */
int acct_ip_count(const torch::Tensor& ips) {
  check_dev(ips, "ips");
  TORCH_CHECK(ips.element_size() == 4, "ips must be 32-bit");
  TORCH_CHECK(ips.numel() <= INT_MAX, "too many addresses");
  return (int)ips.numel();
}

void acct_upsert(torch::Tensor table, torch::Tensor ips, bool reset,
                 torch::Tensor rc) {
  uint32_t mask = acct_table_mask(table);
  int n = acct_ip_count(ips);
  check_dev(rc, "rc");
  TORCH_CHECK(rc.element_size() == 4 && rc.numel() >= n,
              "rc must hold one int32 per address");
  if (n == 0) return;
  bng_launch_acct_upsert(table.data_ptr(), mask, ips.data_ptr(), n,
                         reset ? 1 : 0, rc.data_ptr(), cur_stream());
}

void acct_read(torch::Tensor table, torch::Tensor ips, torch::Tensor out) {
  uint32_t mask = acct_table_mask(table);
  int n = acct_ip_count(ips);
  check_dev(out, "out");
  TORCH_CHECK(nbytes(out) >= (size_t)n * sizeof(bng_acct_entry) &&
              ((uintptr_t)out.data_ptr() & 15) == 0,
              "out must hold one 64-byte entry per address");
  if (n == 0) return;
  bng_launch_acct_read(table.data_ptr(), mask, ips.data_ptr(), n,
                       out.data_ptr(), cur_stream());
}

void acct_delete(torch::Tensor table, torch::Tensor ips, torch::Tensor out) {
  uint32_t mask = acct_table_mask(table);
  int n = acct_ip_count(ips);
  check_dev(out, "out");
  TORCH_CHECK(nbytes(out) >= (size_t)n * sizeof(bng_acct_entry) &&
              ((uintptr_t)out.data_ptr() & 15) == 0,
              "out must hold one 64-byte entry per address");
  if (n == 0) return;
  bng_launch_acct_delete(table.data_ptr(), mask, ips.data_ptr(), n,
                         out.data_ptr(), cur_stream());
}

/* Walled-garden gate.  The packet kernels read rows with 16-B loads and
 * index verdict / out_len / gate / order by packet id or position, so every
 * size is checked here. */
uint32_t wg_table_mask(const torch::Tensor& table) {
  return dev_table_mask(table, sizeof(bng_wg_entry), "wg");
}

void check_wg_common(const torch::Tensor& data, const torch::Tensor& in_len,
                     const torch::Tensor& verdict, const torch::Tensor& gate,
                     const torch::Tensor& cfg, const torch::Tensor& stats) {
  check_dev(data, "data"); check_dev(in_len, "in_len");
  TORCH_CHECK(data.dim() == 2 && data.element_size() == 1,
              "data must be [n, stride] bytes");
  TORCH_CHECK(data.size(0) == in_len.numel() && in_len.element_size() == 2 &&
              in_len.numel() <= INT_MAX,
              "in_len must hold one 16-bit length per row");
  TORCH_CHECK(data.size(1) >= 64 && data.size(1) % 16 == 0 &&
              data.size(1) <= 65535,
              "the walled-garden gate needs a stride that is a multiple of "
              "16, 64..65535");
  TORCH_CHECK(((uintptr_t)data.data_ptr() & 15) == 0,
              "the walled-garden gate needs a 16-byte aligned batch");
  check_dev(verdict, "verdict"); check_dev(gate, "gate");
  check_dev(cfg, "wg_cfg"); check_dev(stats, "stats");
  TORCH_CHECK(verdict.numel() == in_len.numel() &&
              verdict.element_size() == 1 &&
              gate.numel() == in_len.numel() && gate.element_size() == 1,
              "verdict and gate must hold one byte per row");
  TORCH_CHECK(nbytes(cfg) >= sizeof(bng_wg_config) &&
              ((uintptr_t)cfg.data_ptr() & 7) == 0, "wg_cfg too small");
  TORCH_CHECK(nbytes(stats) >= BNG_WG_NSTATS * sizeof(uint64_t),
              "stats too small");
}

void wg_uplink(torch::Tensor data, torch::Tensor in_len,
               torch::Tensor verdict, torch::Tensor out_len,
               torch::Tensor gate, c10::optional<torch::Tensor> order_in,
               torch::Tensor order_out, torch::Tensor table,
               torch::Tensor cfg, torch::Tensor stats) {
  check_wg_common(data, in_len, verdict, gate, cfg, stats);
  check_dev(out_len, "out_len"); check_dev(order_out, "order_out");
  int64_t n = in_len.numel();
  TORCH_CHECK(out_len.element_size() == 2 && out_len.numel() == n,
              "out_len must hold one 16-bit length per row");
  TORCH_CHECK(order_out.element_size() == 4 && order_out.numel() >= n,
              "order_out must hold one int32 per row");
  if (order_in.has_value()) {
    check_dev(*order_in, "order");
    TORCH_CHECK(order_in->element_size() == 4 && order_in->numel() >= n,
                "order must hold one int32 per row");
  }
  uint32_t mask = wg_table_mask(table);
  if (n == 0) return;
  bng_launch_wg_uplink(
      data.data_ptr(), in_len.data_ptr(), verdict.data_ptr(),
      out_len.data_ptr(), gate.data_ptr(),
      order_in.has_value() ? order_in->data_ptr() : nullptr,
      order_out.data_ptr(), (int)n, (int)data.size(1), table.data_ptr(),
      mask, cfg.data_ptr(), stats.data_ptr(), cur_stream());
}

void wg_downlink(torch::Tensor data, torch::Tensor in_len,
                 torch::Tensor verdict, torch::Tensor gate,
                 torch::Tensor table, torch::Tensor cfg,
                 torch::Tensor stats) {
  check_wg_common(data, in_len, verdict, gate, cfg, stats);
  uint32_t mask = wg_table_mask(table);
  int n = (int)in_len.numel();
  if (n == 0) return;
  bng_launch_wg_downlink(data.data_ptr(), in_len.data_ptr(),
                         verdict.data_ptr(), gate.data_ptr(), n,
                         (int)data.size(1), table.data_ptr(), mask,
                         cfg.data_ptr(), stats.data_ptr(), cur_stream());
}

void wg_upsert(torch::Tensor table, torch::Tensor batch, torch::Tensor rc) {
  uint32_t mask = wg_table_mask(table);
  int n = upsert_count(batch, sizeof(bng_wg_entry), rc);
  if (n == 0) return;
  TORCH_CHECK(((uintptr_t)batch.data_ptr() & 7) == 0,
              "batch must be 8-byte aligned");
  bng_launch_wg_upsert(table.data_ptr(), mask, batch.data_ptr(), n,
                       rc.data_ptr(), cur_stream());
}

void wg_delete(torch::Tensor table, torch::Tensor ips) {
  uint32_t mask = wg_table_mask(table);
  int n = acct_ip_count(ips);
  if (n == 0) return;
  bng_launch_wg_delete(table.data_ptr(), mask, ips.data_ptr(), n,
                       cur_stream());
}

/* Fine-grained-coherent pinned host memory for the persistent-service
 * doorbell/rings.  torch's pin_memory allocates COARSE-grained host
 * memory on ROCm: a running kernel caches it and never observes host
 * stores (measured on hardware: the doorbell kernel spun forever) —
 * the service requires hipHostMallocCoherent. */
torch::Tensor alloc_pinned_coherent(int64_t nbytes) {
  void* p = nullptr;
  hipError_t e = hipHostMalloc(&p, (size_t)nbytes,
                               hipHostMallocMapped | hipHostMallocCoherent);
  TORCH_CHECK(e == hipSuccess, "hipHostMalloc(coherent) failed: ",
              hipGetErrorString(e));
  memset(p, 0, (size_t)nbytes);
  return torch::from_blob(p, {nbytes},
                          [](void* q) { (void)hipHostFree(q); },
                          torch::TensorOptions().dtype(torch::kUInt8));
}

/* The device-visible alias of a pinned host pointer (same address
 * under ROCm unified addressing, but ask the runtime rather than
 * assume). */
void* dev_ptr_of(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(!t.is_cuda() && t.is_contiguous(), name,
              " must be a contiguous host tensor");
  void* dp = nullptr;
  hipError_t e = hipHostGetDevicePointer(&dp, t.data_ptr(), 0);
  TORCH_CHECK(e == hipSuccess, name,
              " is not device-mapped pinned memory (allocate via "
              "alloc_pinned_coherent): ", hipGetErrorString(e));
  return dp;
}

/* Persistent DHCP service: launched on its own stream (it never
 * returns until stopped, so it must not share a stream with ordinary
 * work); g_svc_stream declared beside the CU-partition helpers. */


void dhcp_service_start(torch::Tensor ctrl, torch::Tensor req,
                        torch::Tensor in_len, torch::Tensor out_len,
                        torch::Tensor verdict, torch::Tensor scratch,
                        int64_t n_slots_arg, int64_t n_blocks,
                        torch::Tensor ctrs,
                        torch::Tensor subs, torch::Tensor pools,
                        torch::Tensor cfg, torch::Tensor stats) {
  check_dev(scratch, "scratch"); check_dev(subs, "subs");
  check_dev(pools, "pools"); check_dev(cfg, "cfg");
  check_dev(stats, "stats");
  TORCH_CHECK(ctrl.numel() * ctrl.element_size() ==
              (long)sizeof(bng_svc_ctrl), "ctrl must be 64 bytes");
  int n_slots = (int)n_slots_arg;
  check_dev(ctrs, "ctrs");
  TORCH_CHECK(ctrs.numel() * ctrs.element_size() >= 32,
              "ctrs must be >= 32 bytes");
  TORCH_CHECK(n_blocks >= 1 && n_blocks <= 16, "n_blocks in [1,16]");
  if (!g_svc_stream) {
    if (g_svc_cus > 0) {
      uint32_t mask[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      for (int c = 0; c < g_svc_cus; ++c)
        mask[c % 8] |= (1u << (c / 8));
      (void)hipExtStreamCreateWithCUMask(&g_svc_stream, 8, mask);
    } else {
      (void)hipStreamCreateWithFlags(&g_svc_stream, hipStreamNonBlocking);
    }
  }
  bng_launch_dhcp_service(
      dev_ptr_of(ctrl, "ctrl"), dev_ptr_of(req, "req"),
      dev_ptr_of(in_len, "in_len"), dev_ptr_of(out_len, "out_len"),
      dev_ptr_of(verdict, "verdict"), scratch.data_ptr(), n_slots,
      (int)n_blocks, ctrs.data_ptr(),
      subs.data_ptr(), table_mask(subs, sizeof(bng_sub_entry), "subs"),
      pools.data_ptr(),
      (uint32_t)(pools.numel() * pools.element_size() /
                 sizeof(bng_ip_pool)),
      cfg.data_ptr(), stats.data_ptr(), g_svc_stream);
  hipError_t e = hipGetLastError();
  TORCH_CHECK(e == hipSuccess, "dhcp_service launch failed: ",
              hipGetErrorString(e));
}

void dhcp_service_join() {
  if (g_svc_stream) (void)hipStreamSynchronize(g_svc_stream);
}

py::dict layout_report() {
  py::dict d;
#define SZ(T) d[#T] = sizeof(T)
  SZ(bng_sub_entry); SZ(bng_ip_pool); SZ(bng_server_config);
  SZ(bng_nat_tuple); SZ(bng_nat_session); SZ(bng_nat_reverse);
  SZ(bng_eim_entry); SZ(bng_subctx); SZ(bng_nat_config);
  SZ(bng_nat_log_entry); SZ(bng_qos_bucket); SZ(bng_binding_entry);
  SZ(bng_antispoof_config); SZ(bng_spoof_event); SZ(bng_ring_header);
  SZ(bng_svc_ctrl); SZ(bng_sess_export);
  SZ(bng_pppoe_sess); SZ(bng_pppoe_ip); SZ(bng_acct_entry);
  SZ(bng_wg_entry); SZ(bng_wg_config);
#undef SZ
  py::dict off;
  off["sub_entry.lease_expiry"] = offsetof(bng_sub_entry, lease_expiry);
  off["nat_session.last_seen"] = offsetof(bng_nat_session, last_seen);
  off["nat_session.created"] = offsetof(bng_nat_session, created);
  off["nat_session.ready"] = offsetof(bng_nat_session, ready);
  off["eim_entry.created"] = offsetof(bng_eim_entry, created);
  off["subctx.rate_bps"] = offsetof(bng_subctx, rate_bps);
  off["subctx.next_port"] = offsetof(bng_subctx, next_port);
  off["subctx.sessions_active"] = offsetof(bng_subctx, sessions_active);
  off["qos_bucket.tokens"] = offsetof(bng_qos_bucket, tokens);
  off["qos_bucket.last_update"] = offsetof(bng_qos_bucket, last_update);
  off["binding_entry.ipv6_addr"] = offsetof(bng_binding_entry, ipv6_addr);
  off["nat_config.priv_lo"] = offsetof(bng_nat_config, priv_lo);
  off["nat_config.alg_key"] = offsetof(bng_nat_config, alg_key);
  off["antispoof_config.allowed_lo"] =
      offsetof(bng_antispoof_config, allowed_lo);
  off["spoof_event.spoofed_ip"] = offsetof(bng_spoof_event, spoofed_ip);
  off["pppoe_sess.ip"] = offsetof(bng_pppoe_sess, ip);
  off["pppoe_sess.mru"] = offsetof(bng_pppoe_sess, mru);
  off["pppoe_sess.session_id"] = offsetof(bng_pppoe_sess, session_id);
  off["pppoe_ip.sid_mac"] = offsetof(bng_pppoe_ip, sid_mac);
  off["acct_entry.up_bytes"] = offsetof(bng_acct_entry, up_bytes);
  off["acct_entry.down_bytes"] = offsetof(bng_acct_entry, down_bytes);
  off["acct_entry.up_drop_pkts"] = offsetof(bng_acct_entry, up_drop_pkts);
  off["acct_entry.last_seen"] = offsetof(bng_acct_entry, last_seen);
  off["wg_entry.mac_state"] = offsetof(bng_wg_entry, mac_state);
  off["wg_config.allowed_key"] = offsetof(bng_wg_config, allowed_key);
  off["wg_config.allowed_ip"] = offsetof(bng_wg_config, allowed_ip);
  off["wg_config.redirect_port"] = offsetof(bng_wg_config, redirect_port);
  d["offsets"] = off;
  return d;
}

/* Peel rounds of the accounting commit's wave-level combining: 0 = none,
 * < 0 = until nothing is pending.  The A/B knob of scripts/acct_bench.py;
 * tests use it to run every variant over the same batches. */
void set_acct_combine(int64_t rounds) {
  TORCH_CHECK(rounds >= -1 && rounds <= 64, "rounds in [-1,64]");
  bng_set_acct_combine((int)rounds);
}

int64_t get_acct_combine() { return bng_get_acct_combine(); }

/* Grid cap (in 256-thread blocks) of the batched packet kernels; 0
 * restores the built-in default.  The A/B knob for grid sizing, and the
 * hook tests use to force several grid-stride iterations at tiny n. */
void set_pkt_grid_cap(int64_t blocks) {
  TORCH_CHECK(blocks >= 0 && blocks <= 65536, "blocks in [0,65536]");
  bng_set_pkt_grid_cap((int)blocks);
}

int64_t get_pkt_grid_cap() { return bng_get_pkt_grid_cap(); }

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("dhcp_fastpath", &dhcp_fastpath,
        py::arg("data"), py::arg("in_len"), py::arg("out_len"),
        py::arg("verdict"), py::arg("subs"), py::arg("pools"),
        py::arg("cfg"), py::arg("stats"), py::arg("now_sec"),
        py::arg("now_buf") = py::none());
  m.def("nat44", &nat44);
  m.def("qos", &qos);
  m.def("antispoof", &antispoof);
  m.def("uplink_pipeline", &uplink_pipeline,
        py::arg("data"), py::arg("in_len"), py::arg("out_len"),
        py::arg("verdict"), py::arg("subs"), py::arg("pools"),
        py::arg("scfg"), py::arg("dhcp_stats"), py::arg("bindings"),
        py::arg("acfg"), py::arg("as_stats"), py::arg("spoof_ring"),
        py::arg("spoof_hdr"), py::arg("sessions"), py::arg("reverse"),
        py::arg("eim"), py::arg("subctx"), py::arg("ncfg"),
        py::arg("hairpin"), py::arg("n_hairpin"), py::arg("nat_stats"),
        py::arg("log_ring"), py::arg("log_hdr"), py::arg("qos_eg"),
        py::arg("qos_stats"), py::arg("now_ns"), py::arg("now_sec"),
        py::arg("order") = py::none(),
        py::arg("downlink") = false,
        py::arg("now_buf") = py::none(),
        py::arg("masked") = false);
  m.def("set_cu_partition", &set_cu_partition);
  m.def("masked_sync", &masked_sync);
  m.def("pkt_class", &pkt_class);
  m.def("sub_upsert", &sub_upsert);
  m.def("sub_delete", &sub_delete);
  m.def("sess_import", &sess_import);
  m.def("subctx_upsert", &subctx_upsert);
  m.def("qos_upsert", &qos_upsert);
  m.def("binding_upsert", &binding_upsert);
  m.def("binding_delete", &binding_delete);
  m.def("pppoe_decap", &pppoe_decap);
  m.def("pppoe_encap", &pppoe_encap);
  m.def("pppoe_sess_upsert", &pppoe_sess_upsert);
  m.def("pppoe_sess_delete", &pppoe_sess_delete);
  m.def("acct_resolve", &acct_resolve);
  m.def("acct_commit", &acct_commit);
  m.def("acct_downlink", &acct_downlink);
  m.def("acct_upsert", &acct_upsert);
  m.def("acct_read", &acct_read);
  m.def("acct_delete", &acct_delete);
  m.def("wg_uplink", &wg_uplink, py::arg("data"), py::arg("in_len"),
        py::arg("verdict"), py::arg("out_len"), py::arg("gate"),
        py::arg("order_in"), py::arg("order_out"), py::arg("table"),
        py::arg("cfg"), py::arg("stats"));
  m.def("wg_downlink", &wg_downlink);
  m.def("wg_upsert", &wg_upsert);
  m.def("wg_delete", &wg_delete);
  m.def("set_acct_combine", &set_acct_combine, py::arg("rounds"));
  m.def("get_acct_combine", &get_acct_combine);
  m.def("nat_sweep", &nat_sweep);
  m.def("shard_owner", &shard_owner);
  m.def("dhcp_service_start", &dhcp_service_start);
  m.def("alloc_pinned_coherent", &alloc_pinned_coherent);
  m.def("dhcp_service_join", &dhcp_service_join);
  m.def("layout_report", &layout_report);
  m.def("set_pkt_grid_cap", &set_pkt_grid_cap, py::arg("blocks"));
  m.def("get_pkt_grid_cap", &get_pkt_grid_cap);
}
