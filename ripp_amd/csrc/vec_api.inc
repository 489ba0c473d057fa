// Included by engine.hip inside its `extern "C"` block (after tipa_api.inc: it reuses fold_dev and the VM fall-back driver).
// ---- device-resident vectors (SURVEY.md section 8b: `ripp_vec`) -----------------------------------------------------------------------
// The trait-level entry points above take HOST slices, as the reference's traits do: every call uploads, normalises and downloads.  A
// generic GIPA through those traits (gipa.rs:196-297) therefore moves each vector six times per round.  A ripp_vec keeps a vector in HBM
// across calls: group elements AFFINE (normalised once, on upload or after a fold -- the same normalisation every commitment of the
// reference starts with, inner_products/src/lib.rs:80-81), scalars in Montgomery form.  Halves and slices are VIEWS sharing the storage
// (reference-counted), so `m_a[split..]` / `ck_a[..split]` of a round cost nothing; the inner products, the commitments built from them
// and the folds read the views in place.
extern "C++" {
struct VecStore { void* p = nullptr; size_t bytes = 0; ~VecStore() { if (p) { (void)hipFree(p); g_dev_bytes.fetch_sub(bytes, std::memory_order_relaxed); } } };      // counted like a DevBuf (ripp_device_bytes, mem_cap_bytes)
}
struct ripp_vec { int32_t kind = 0; std::shared_ptr<VecStore> st; size_t off = 0, len = 0; };
extern "C++" {
static size_t vec_elem_size(int32_t kind) { return kind == RIPP_VEC_G1 ? sizeof(G1A) : kind == RIPP_VEC_G2 ? sizeof(G2A) : sizeof(Fr); }
template <class T> static T* vec_ptr(const ripp_vec* v) { return reinterpret_cast<T*>(v->st->p) + v->off; }
static int32_t vec_alloc(int32_t kind, size_t n, ripp_vec** out) {
    auto st = std::make_shared<VecStore>();
    const size_t bytes = std::max<size_t>(n, 1) * vec_elem_size(kind);
    HIPCHK(hipMalloc(&st->p, bytes)); st->bytes = bytes; g_dev_bytes.fetch_add(bytes, std::memory_order_relaxed);
    ripp_vec* v = new ripp_vec; v->kind = kind; v->st = std::move(st); v->off = 0; v->len = n;
    ++g_live_handles; *out = v; return RIPP_OK;
}
static void vec_drop(ripp_vec* v) { if (v) { delete v; --g_live_handles; } }
template <class F, bool JAC> static int32_t vec_upload_pts(int32_t kind, const void* host, size_t n, ripp_vec** out) {
    if (!out || (n && !host)) return RIPP_ERR_ARG;
    LOCK; ENGINE;
    ripp_vec* v; int32_t rc = vec_alloc(kind, n, &v); if (rc) return rc;
    if (n) {
        if (JAC) {
            DevBuf& jac = std::is_same<F, Fp>::value ? e->jacG1 : e->jacG2;
            Jac<F>* dj; if ((rc = upload<Jac<F>>(e, jac, host, n, &dj)) || (rc = e->normalize_dev<F>(dj, n, vec_ptr<Affine<F>>(v)))) { vec_drop(v); return rc; }
        } else if (hipMemcpyAsync(v->st->p, host, n * sizeof(Affine<F>), hipMemcpyHostToDevice, e->stream) != hipSuccess) { vec_drop(v); set_err("ripp_vec_upload: hipMemcpyAsync failed"); return RIPP_ERR_DEVICE; }
        if ((rc = e->sync())) { vec_drop(v); return rc; }          // the host slice is the caller's again when this returns
    }
    *out = v; return RIPP_OK;
}
static int32_t fr_dot_dev(Engine* e, const Fr* dl, const Fr* dr, size_t n, Fr* acc_out) {
    Fr acc = Fr::zero();
    if (n) {
        const unsigned blocks = std::min<unsigned>(1024, nblk(n, 256));
        int32_t rc; if ((rc = e->tmpB.reserve(blocks * sizeof(Fr)))) return rc;
        hipLaunchKernelGGL(k_fr_dot, dim3(blocks), dim3(256), 0, e->stream, dl, dr, (uint32_t)n, e->tmpB.as<Fr>());
        HIPCHK(hipGetLastError());
        std::vector<Fr> part(blocks);
        HIPCHK(hipMemcpyAsync(part.data(), e->tmpB.p, blocks * sizeof(Fr), hipMemcpyDeviceToHost, e->stream));
        if ((rc = e->sync())) return rc;
        for (const Fr& p : part) acc = add(acc, p);
    }
    *acc_out = acc; return RIPP_OK;
}
static int32_t vec_len_err(size_t l, size_t r) { set_err("left length, right length: " + std::to_string(l) + ", " + std::to_string(r)); return RIPP_ERR_LENGTH; }
}  // extern "C++"

API int32_t ripp_vec_upload_g1a(const ripp_g1a* p, size_t n, ripp_vec** out) { return vec_upload_pts<Fp, false>(RIPP_VEC_G1, p, n, out); }
API int32_t ripp_vec_upload_g2a(const ripp_g2a* p, size_t n, ripp_vec** out) { return vec_upload_pts<Fp2, false>(RIPP_VEC_G2, p, n, out); }
API int32_t ripp_vec_upload_g1j(const ripp_g1j* p, size_t n, ripp_vec** out) { return vec_upload_pts<Fp, true>(RIPP_VEC_G1, p, n, out); }
API int32_t ripp_vec_upload_g2j(const ripp_g2j* p, size_t n, ripp_vec** out) { return vec_upload_pts<Fp2, true>(RIPP_VEC_G2, p, n, out); }
API int32_t ripp_vec_upload_fr(const ripp_fr* p, size_t n, ripp_vec** out) {
    if (!out || (n && !p)) return RIPP_ERR_ARG;
    LOCK; ENGINE;
    ripp_vec* v; int32_t rc = vec_alloc(RIPP_VEC_FR, n, &v); if (rc) return rc;
    if (n && (hipMemcpyAsync(v->st->p, p, n * sizeof(Fr), hipMemcpyHostToDevice, e->stream) != hipSuccess || e->sync())) { vec_drop(v); set_err("ripp_vec_upload_fr: copy failed"); return RIPP_ERR_DEVICE; }
    *out = v; return RIPP_OK;
}
API size_t ripp_vec_len(const ripp_vec* v) { return v ? v->len : 0; }
API int32_t ripp_vec_kind(const ripp_vec* v) { return v ? v->kind : 0; }
API void ripp_vec_free(ripp_vec* v) { if (!v) return; LOCK; vec_drop(v); }
// view of elements [off, off + len): shares the storage, freed independently (the storage goes with its last view)
API int32_t ripp_vec_slice(const ripp_vec* v, size_t off, size_t len, ripp_vec** out) {
    if (!v || !out || off > v->len || len > v->len - off) return RIPP_ERR_ARG;
    LOCK;
    ripp_vec* s = new ripp_vec(*v); s->off = v->off + off; s->len = len; ++g_live_handles; *out = s; return RIPP_OK;
}
// (lo, hi) = (v[..len/2], v[len/2..]) -- the split of a halving round (gipa.rs:207-217, sipp/src/lib.rs:71-75)
API int32_t ripp_vec_halves(const ripp_vec* v, ripp_vec** lo, ripp_vec** hi) {
    if (!v || !lo || !hi || (v->len & 1)) return RIPP_ERR_ARG;
    int32_t rc = ripp_vec_slice(v, 0, v->len / 2, lo); if (rc) return rc;
    if ((rc = ripp_vec_slice(v, v->len / 2, v->len / 2, hi))) { ripp_vec_free(*lo); *lo = nullptr; }
    return rc;
}
// elements back to the host: ripp_g1a / ripp_g2a / ripp_fr by kind
API int32_t ripp_vec_download(const ripp_vec* v, void* out) {
    if (!v || (v->len && !out)) return RIPP_ERR_ARG;
    LOCK; ENGINE; if (v->len == 0) return RIPP_OK;
    const size_t es = vec_elem_size(v->kind);
    HIPCHK(hipMemcpyAsync(out, static_cast<const char*>(v->st->p) + v->off * es, v->len * es, hipMemcpyDeviceToHost, e->stream));
    return e->sync();
}
// PairingInnerProduct::inner_product on resident vectors (inner_products/src/lib.rs:61-73)
API int32_t ripp_vec_pairing_product(const ripp_vec* left, const ripp_vec* right, ripp_gt* out) {
    if (!left || !right || !out || left->kind != RIPP_VEC_G1 || right->kind != RIPP_VEC_G2) return RIPP_ERR_ARG;
    if (left->len != right->len) return vec_len_err(left->len, right->len);
    LOCK; ENGINE;
    return pairing_product_dev(e, vec_ptr<G1A>(left), vec_ptr<G2A>(right), left->len, out);
}
// MultiexponentiationInnerProduct::inner_product (inner_products/src/lib.rs:128-141): out is a ripp_g1j or ripp_g2j by the bases' kind
API int32_t ripp_vec_msm(const ripp_vec* bases, const ripp_vec* scalars, void* out) {
    if (!bases || !scalars || !out || scalars->kind != RIPP_VEC_FR || (bases->kind != RIPP_VEC_G1 && bases->kind != RIPP_VEC_G2)) return RIPP_ERR_ARG;
    if (bases->len != scalars->len) return vec_len_err(bases->len, scalars->len);
    LOCK; ENGINE;
    if (bases->kind == RIPP_VEC_G1) {
        G1J res = jac_inf<Fp>(); int32_t rc;
        if (bases->len && (rc = e->msm_dev<Fp>(vec_ptr<G1A>(bases), vec_ptr<Fr>(scalars), bases->len, &res))) return rc;
        std::memcpy(out, &res, sizeof res);
    } else {
        G2J res = jac_inf<Fp2>(); int32_t rc;
        if (bases->len && (rc = e->msm_dev<Fp2>(vec_ptr<G2A>(bases), vec_ptr<Fr>(scalars), bases->len, &res))) return rc;
        std::memcpy(out, &res, sizeof res);
    }
    return RIPP_OK;
}
// ScalarInnerProduct::inner_product (inner_products/src/lib.rs:144-166)
API int32_t ripp_vec_scalar_inner_product(const ripp_vec* left, const ripp_vec* right, ripp_fr* out) {
    if (!left || !right || !out || left->kind != RIPP_VEC_FR || right->kind != RIPP_VEC_FR) return RIPP_ERR_ARG;
    if (left->len != right->len) return vec_len_err(left->len, right->len);
    LOCK; ENGINE;
    Fr acc; int32_t rc = fr_dot_dev(e, vec_ptr<Fr>(left), vec_ptr<Fr>(right), left->len, &acc); if (rc) return rc;
    std::memcpy(out, &acc, sizeof acc); return RIPP_OK;
}
// the fold of a halving round, device to device: out[i] = s * hi[i] + lo[i]  (gipa.rs:262-291; group kinds come back normalised)
API int32_t ripp_vec_fold(const ripp_vec* hi, const ripp_vec* lo, const ripp_fr* s, ripp_vec** out) {
    if (!hi || !lo || !s || !out || hi->kind != lo->kind) return RIPP_ERR_ARG;
    if (hi->len != lo->len) return vec_len_err(hi->len, lo->len);
    LOCK; ENGINE;
    const size_t half = hi->len;
    Fr sm; std::memcpy(&sm, s, sizeof sm);
    ripp_vec* v; int32_t rc = vec_alloc(hi->kind, half, &v); if (rc) return rc;
    if (half) {
        if (hi->kind == RIPP_VEC_FR) {
            hipLaunchKernelGGL(k_fold_fr, dim3(nblk(half, 256)), dim3(256), 0, e->stream, vec_ptr<Fr>(hi), vec_ptr<Fr>(lo), (uint32_t)half, sm, vec_ptr<Fr>(v));
            rc = hipGetLastError() == hipSuccess ? e->sync() : RIPP_ERR_DEVICE;
        } else if (e->cfg.pub.no_endo) {                              // builds / switches without the endomorphisms: the plain NAF fold
            if (hi->kind == RIPP_VEC_G1) {
                if (!(rc = e->jacG1.reserve(half * sizeof(G1J)))) {
                    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_fold_affine_naf<Fp>), dim3(nblk(half, 256)), dim3(256), 0, e->stream, vec_ptr<G1A>(hi), vec_ptr<G1A>(lo), (uint32_t)half, naf_digits(sm), e->jacG1.as<G1J>());
                    if (!(rc = e->normalize_dev<Fp>(e->jacG1.as<G1J>(), half, vec_ptr<G1A>(v)))) rc = e->sync();
                }
            } else if (!(rc = e->jacG2.reserve(half * sizeof(G2J)))) {
                hipLaunchKernelGGL(HIP_KERNEL_NAME(k_fold_affine_naf<Fp2>), dim3(nblk(half, 256)), dim3(256), 0, e->stream, vec_ptr<G2A>(hi), vec_ptr<G2A>(lo), (uint32_t)half, naf_digits(sm), e->jacG2.as<G2J>());
                if (!(rc = e->normalize_dev<Fp2>(e->jacG2.as<G2J>(), half, vec_ptr<G2A>(v)))) rc = e->sync();
            }
        } else if (hi->kind == RIPP_VEC_G1) {
            rc = fork_join_folds(e, [&]() { return fold_dev<Fp>(e, e->stream, vec_ptr<G1A>(hi), vec_ptr<G1A>(lo), half, sm, e->jacG1, e->qtab, vec_ptr<G1A>(v)); });
        } else {
            rc = fork_join_folds(e, [&]() { return fold_dev<Fp2>(e, e->stream, vec_ptr<G2A>(hi), vec_ptr<G2A>(lo), half, sm, e->jacG2, e->qtab, vec_ptr<G2A>(v)); });
        }
        if (rc) { vec_drop(v); return rc; }
    }
    *out = v; return RIPP_OK;
}
