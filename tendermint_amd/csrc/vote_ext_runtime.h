// Vote-extension entries of a device-built batch
// (tmv_verify_votes_and_extensions): included by tmverify_runtime.cpp twice,
// TMV_VOTE_EXT_PART 1 before stage_whole (the staging of a chunk's
// extension entries) and 2 after run_batch (the C ABI).
//
// A batch holds n_votes vote entries, then n_exts extension entries.  A chunk
// [lo, hi) of it stages, after the vote templates:
//   extension templates (VoteExtTab[], tails) | template index per entry |
//   payload offsets (ne + 1) | payloads + 16 spare bytes
// Payloads are in entry order, so the chunk's payloads are one contiguous
// span of ext_data.  Per extension entry 8 bytes (template index, payload
// offset) and its payload cross PCIe; the messages are written on the device.
#if TMV_VOTE_EXT_PART == 1

struct VoteExtSrc {
  uint32_t n_votes;    // entries [0, n_votes) of the batch are vote entries
  const uint8_t *tab;  // n_etmpl VoteExtTab, then the tails
  size_t tab_bytes, blob_at;
  const uint32_t *tmpl;  // per extension entry
  const uint8_t *data;
  const uint32_t *off;  // n_exts + 1
  uint32_t n_exts;
};

// Where a chunk's extension entries sit in the lane's staging.
struct VoteExtStage {
  uint32_t nv = 0, ne = 0, e0 = 0;  // vote entries, extension entries, first extension entry
  size_t tab_at = 0, idx_at = 0, off_at = 0, data_at = 0, data_bytes = 0, end = 0;
};

// The payload region starts 16-byte aligned and ends with 16 spare bytes:
// wave_copy (signbytes_kernels.hip) loads the aligned dwords around a payload.
static VoteExtStage vote_ext_plan(const VoteExtSrc *x, uint32_t lo, uint32_t hi, size_t at) {
  VoteExtStage p;
  p.nv = hi - lo;
  p.end = at;
  if (!x) return p;
  p.nv = lo < x->n_votes ? std::min(hi, x->n_votes) - lo : 0;
  p.ne = (hi - lo) - p.nv;
  if (!p.ne) return p;
  p.e0 = std::max(lo, x->n_votes) - x->n_votes;
  p.tab_at = at;
  p.idx_at = p.tab_at + align16(x->tab_bytes);
  p.off_at = p.idx_at + align16(4ull * p.ne);
  p.data_at = p.off_at + align16(4ull * (p.ne + 1));
  p.data_bytes = (size_t)x->off[p.e0 + p.ne] - x->off[p.e0];
  p.end = p.data_at + align16(p.data_bytes) + 16;
  return p;
}

static void vote_ext_stage(const VoteExtSrc &x, const VoteExtStage &p, uint8_t *h) {
  if (!p.ne) return;
  std::memcpy(h + p.tab_at, x.tab, x.tab_bytes);
  std::memcpy(h + p.idx_at, x.tmpl + p.e0, 4ull * p.ne);
  uint32_t *o = reinterpret_cast<uint32_t *>(h + p.off_at);
  const uint32_t base = x.off[p.e0];
  for (uint32_t j = 0; j <= p.ne; j++) o[j] = x.off[p.e0 + j] - base;
  if (p.data_bytes) par_memcpy(h + p.data_at, x.data + base, p.data_bytes);
}

// Read on every launch: tools/bench_vote_ext.py alternates it in one process.
static uint32_t vote_ext_wave_min() {
  const char *e = getenv("TMV_VOTE_EXT_WAVE_MIN");
  return e ? (uint32_t)strtoul(e, nullptr, 10) : tmv::kVoteExtWaveMin;
}

// dd: the staged chunk on the device; doff: the chunk's message offsets
// (entry p.nv is the first extension entry); msg: the message region.
static hipError_t vote_ext_launch(const VoteExtSrc &x, const VoteExtStage &p, const uint8_t *dd,
                                  const uint32_t *doff, uint8_t *msg, hipStream_t s) {
  if (!p.ne) return hipSuccess;
  return tmv::launch_vote_ext_signbytes(reinterpret_cast<const tmv::VoteExtTab *>(dd + p.tab_at),
                                        dd + p.tab_at + x.blob_at,
                                        reinterpret_cast<const uint32_t *>(dd + p.idx_at),
                                        reinterpret_cast<const uint32_t *>(dd + p.off_at), dd + p.data_at,
                                        doff + p.nv, p.ne, msg, vote_ext_wave_min(), s);
}

#elif TMV_VOTE_EXT_PART == 2

// Template table + tails for k_vote_ext_signbytes, and the offsets of the
// extension messages appended to off (which ends with the vote messages'
// total), sized with the device's own length functions.
static int prepare_vote_exts(const tmv_vote_ext_template *etmpl, uint32_t n_etmpl, const uint32_t *ext_tmpl,
                             const uint8_t *ext_data, const uint32_t *ext_off, uint32_t n_exts,
                             std::vector<uint8_t> &tab, size_t &blob_at, std::vector<uint32_t> &off) {
  if ((!etmpl && n_etmpl) || (n_exts && (!ext_tmpl || !ext_off))) { set_error("null argument"); return TMV_ERR_ARG; }
  std::vector<tmv::VoteExtTab> vt(n_etmpl);
  uint64_t blob = 0;
  for (uint32_t t = 0; t < n_etmpl; t++) {
    if (etmpl[t].tail_len && !etmpl[t].tail) { set_error("null template segment"); return TMV_ERR_ARG; }
    vt[t] = tmv::VoteExtTab{(uint32_t)blob, etmpl[t].tail_len};
    blob += etmpl[t].tail_len;
    if (blob > (1u << 30)) { set_error("vote extension templates too large"); return TMV_ERR_ARG; }
  }
  blob_at = align16(sizeof(tmv::VoteExtTab) * n_etmpl);
  tab.resize(blob_at + blob);
  if (n_etmpl) std::memcpy(tab.data(), vt.data(), sizeof(tmv::VoteExtTab) * n_etmpl);
  for (uint32_t t = 0; t < n_etmpl; t++)
    if (vt[t].tail_len) std::memcpy(tab.data() + blob_at + vt[t].tail_at, etmpl[t].tail, vt[t].tail_len);
  const size_t n0 = off.size() - 1;
  if ((uint64_t)n0 + n_exts > UINT32_MAX - 1) { set_error("too many entries"); return TMV_ERR_ARG; }
  off.resize(n0 + n_exts + 1);
  if (!n_exts) return 0;
  if (ext_off[0] != 0) { set_error("ext_off[0] must be 0"); return TMV_ERR_ARG; }
  uint64_t acc = off[n0];
  for (uint32_t j = 0; j < n_exts; j++) {
    if (ext_tmpl[j] >= n_etmpl) { set_error("vote extension template index out of range"); return TMV_ERR_ARG; }
    if (ext_off[j + 1] < ext_off[j]) { set_error("ext_off must not decrease"); return TMV_ERR_ARG; }
    acc += tmv::vote_ext_msg_len(vt[ext_tmpl[j]].tail_len, ext_off[j + 1] - ext_off[j]);
    if (acc > UINT32_MAX) { set_error("vote messages exceed 4 GiB"); return TMV_ERR_ARG; }
    off[n0 + j + 1] = (uint32_t)acc;
  }
  if (ext_off[n_exts] && !ext_data) { set_error("null argument"); return TMV_ERR_ARG; }
  return 0;
}

extern "C" {

int tmv_verify_votes_and_extensions(tmv_ctx *ctx, uint8_t key_kind, uint32_t flags, const tmv_vote_template *tmpl,
                                    uint32_t n_tmpl, const tmv_vote *votes, uint32_t n_votes,
                                    const tmv_vote_ext_template *etmpl, uint32_t n_etmpl, const uint32_t *ext_tmpl,
                                    const uint8_t *ext_data, const uint32_t *ext_off, uint32_t n_exts,
                                    const uint8_t *pk, const uint8_t *sig, int8_t *status_out) {
  if (!ctx) { set_error("null context"); return TMV_ERR_ARG; }
  const bool cache = (flags & TMV_FLAG_KEY_CACHE) != 0;
  Scheme sch;
  if (key_kind == TMV_KIND_ED25519) sch = cache ? Scheme::Ed25519Cached : Scheme::Ed25519;
  else if (key_kind == TMV_KIND_SR25519) sch = cache ? Scheme::Sr25519Cached : Scheme::Sr25519;
  else { set_error("unsupported key kind"); return TMV_ERR_ARG; }
  if ((uint64_t)n_votes + n_exts > UINT32_MAX - 1) { set_error("too many entries"); return TMV_ERR_ARG; }
  static thread_local std::vector<uint8_t> tab, etab;
  static thread_local std::vector<uint32_t> off;
  size_t blob_at = 0, eblob_at = 0;
  EngineTimer tm;
  int pr = prepare_votes(tmpl, n_tmpl, votes, n_votes, tab, blob_at, off);
  if (pr < 0) return pr;
  pr = prepare_vote_exts(etmpl, n_etmpl, ext_tmpl, ext_data, ext_off, n_exts, etab, eblob_at, off);
  if (pr < 0) return pr;
  tm.mark("votes + extensions", n_votes + n_exts);
  const VoteExtSrc xs{n_votes, etab.data(), etab.size(), eblob_at, ext_tmpl, ext_data, ext_off, n_exts};
  const VoteSrc vs{votes, tab.data(), tab.size(), blob_at, &xs};
  return run_batch(ctx, sch, nullptr, pk, sig, nullptr, off.data(), n_votes + n_exts,
                   reinterpret_cast<uint8_t *>(status_out), flags, &vs);
}

int64_t tmv_vote_extension_sign_bytes_device(tmv_ctx *ctx, const tmv_vote_ext_template *etmpl, uint32_t n_etmpl,
                                             const uint32_t *ext_tmpl, const uint8_t *ext_data,
                                             const uint32_t *ext_off, uint32_t n_exts, uint8_t *msg_out,
                                             size_t msg_cap, uint32_t *msg_off_out) {
  if (!ctx || !msg_off_out) { set_error("null argument"); return TMV_ERR_ARG; }
  std::vector<uint8_t> etab;
  std::vector<uint32_t> off(1, 0);
  size_t eblob_at = 0;
  const int pr = prepare_vote_exts(etmpl, n_etmpl, ext_tmpl, ext_data, ext_off, n_exts, etab, eblob_at, off);
  if (pr < 0) return pr;
  std::memcpy(msg_off_out, off.data(), sizeof(uint32_t) * ((size_t)n_exts + 1));
  const size_t total = off[n_exts];
  if (!msg_out || n_exts == 0) return (int64_t)total;
  if (msg_cap < total) { set_error("msg_cap too small"); return TMV_ERR_ARG; }
  const VoteExtSrc xs{0, etab.data(), etab.size(), eblob_at, ext_tmpl, ext_data, ext_off, n_exts};
  const VoteExtStage p = vote_ext_plan(&xs, 0, n_exts, 0);
  const size_t o_at = p.end, m_at = o_at + align16(4ull * (n_exts + 1)), bytes = m_at + total;
  std::vector<uint8_t> h(m_at);
  vote_ext_stage(xs, p, h.data());
  std::memcpy(h.data() + o_at, off.data(), 4ull * (n_exts + 1));
  Device &d = *ctx->devs[0];
  std::lock_guard<std::mutex> lk(d.mu);
  if (d.faulted) return faulted_rc(d);
  hipStream_t s;
  int rc = use_device(d, nullptr, &s);
  if (rc != 0) return rc;
  uint8_t *dev = nullptr;
  hipError_t e;
  if ((e = hipMalloc(&dev, bytes)) != hipSuccess) { set_error("hipMalloc", e); return TMV_ERR_NOMEM; }
  if ((e = hipMemcpyAsync(dev, h.data(), m_at, hipMemcpyHostToDevice, s)) != hipSuccess ||
      (e = vote_ext_launch(xs, p, dev, reinterpret_cast<const uint32_t *>(dev + o_at), dev + m_at, s)) !=
          hipSuccess ||
      (e = hipMemcpyAsync(msg_out, dev + m_at, total, hipMemcpyDeviceToHost, s)) != hipSuccess ||
      (e = wait_stream(d, s)) != hipSuccess) {
    if (e != hipErrorNotReady) set_error("tmv_vote_extension_sign_bytes_device", e);
    rc = wait_rc(e);
  }
  if (!d.faulted) (void)hipFree(dev);
  return rc < 0 ? rc : (int64_t)total;
}

}  // extern "C"

#endif
