// Device test harness for the stages of the Pippenger MSM behind the digit pass (ripp_amd/csrc/msm.hpp, msm_batch.hpp): the counting sort (k_msm_hist_lds, k_msm_scan,
// k_msm_scatter_lds, k_msm_scatter), the grouping passes and the bucket merge (k_msm_slot_group, k_msm_vm_merge, k_msm_bucket_merge), the segment sums and their
// tree (k_msm_vm_segments, k_msm_segments, k_msm_vm_reduce, k_msm_seg_reduce) and the Horner finish (k_msm_finish_vm, k_msm_finish, k_msm_finish_vm_batch).
// The gathered additions (k_msm_extend_q, k_msm_slot_sum*) are in msm_slot_edges.hip.  The production headers are included unchanged; every entry launches ONE
// stage with the grid, block and dynamic-LDS expressions of engine.hip (Engine::msm_launch / Engine::msm_batch_dev), quoted at each launch.
// tests/test_gpu_msm_edges.py feeds it the inputs of tests/msm_edges.py and compares every result with Python integers.
//
// Built twice by tests/device/Makefile: libmsm_edges_381.so and libmsm_edges_377.so (-DRIPP_BLS12_377).  Every entry takes HOST arrays, copies them to the device,
// launches, waits and copies back; it returns the HIP error code (0 = success, -1 = refused arguments, msm_edges_util.hpp).  The plan is 8 words (c, nwin, nb, n, ch,
// seg, nreal, gmin), so a test picks c, nwin, ch and gmin freely and nwin may be a batch's virtual windows.  Every output array has MS_SLACK elements of slack, is
// filled with MS_SENTINEL words before the launch and is returned whole.  Points are the engine's: Jac<Fp> = 36 words, Jac<Fp2> = 72 words, Montgomery form.
#include "msm_edges_util.hpp"

using namespace ripp;
using namespace msedge;

static_assert(sizeof(G1J) == 144 && sizeof(G2J) == 288, "struct sizes the Python side packs");

namespace {
template <class F> constexpr size_t jw() { return sizeof(Jac<F>) / 4; }
template <class F> constexpr size_t vm_lds4() { return 4 * VM_EPW * VmCurve<F>::SLOTS * sizeof(VmSlot); }       // engine.hip: const size_t vm_lds = 4 * VM_EPW * VmCurve<F>::SLOTS * sizeof(VmSlot);
template <class F> constexpr size_t vm_lds1() { return VM_EPW * VmCurve<F>::SLOTS * sizeof(VmSlot); }
static_assert(vm_lds4<Fp>() <= 65536 && vm_lds4<Fp2>() <= 65536, "the VM workspace of a 256-lane block fits the LDS");

template <class F> int group_(const MsmPlan& p, const uint32_t* hist, const uint32_t* slot_offs, const uint32_t* spw, uint32_t* slots, uint32_t max_slots, uint32_t stride, int hom) {
    const size_t nwb = (size_t)p.nwin * p.nb, ns = (size_t)p.nwin * max_slots + MS_SLACK;
    DevBuf dh, dso, dsp, dsl;
    MS_CHK(dh.put(hist, nwb * 4)); MS_CHK(dso.put(slot_offs, nwb * 4)); MS_CHK(dsp.put(spw, (size_t)p.nwin * 4)); MS_CHK(dsl.put(slots, ns * sizeof(Jac<F>)));
    // engine.hip: hipLaunchKernelGGL(HIP_KERNEL_NAME(k_msm_slot_group<F>), dim3(nblk(max_slots, 64), p.nwin), dim3(64), 0, st, p, ms.hist.as<uint32_t>(),
    //                                ms.slotoffs.as<uint32_t>(), ms.spw.as<uint32_t>(), ms.slots.as<Jac<F>>(), max_slots, stride, hom);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_msm_slot_group<F>), dim3(nblk(max_slots, 64), p.nwin), dim3(64), 0, 0, p, dh.as<uint32_t>(), dso.as<uint32_t>(), dsp.as<uint32_t>(),
                       dsl.as<Jac<F>>(), max_slots, stride, hom != 0);
    MS_CHK(hipGetLastError()); MS_CHK(hipDeviceSynchronize());
    MS_CHK(dsl.get(slots, ns * sizeof(Jac<F>)));
    return 0;
}
template <class F> int merge_(int kind, const MsmPlan& p, const uint32_t* hist, const uint32_t* slot_offs, const uint32_t* slots, uint32_t max_slots, uint32_t passes, int hom, uint32_t* buckets) {
    const size_t nwb = (size_t)p.nwin * p.nb;
    DevBuf dh, dso, dsl, db;
    MS_CHK(dh.put(hist, nwb * 4)); MS_CHK(dso.put(slot_offs, nwb * 4)); MS_CHK(dsl.put(slots, (size_t)p.nwin * max_slots * sizeof(Jac<F>)));
    MS_CHK(db.sentinel((nwb + MS_SLACK) * jw<F>()));
    if (kind == 0)
        // engine.hip: hipLaunchKernelGGL(HIP_KERNEL_NAME(k_msm_vm_merge<F>), dim3(nblk(p.nb, 4 * VM_EPW), p.nwin), dim3(256), vm_lds, st, p, ms.hist.as<uint32_t>(), ms.slotoffs.as<uint32_t>(),
        //                                ms.slots.as<Jac<F>>(), max_slots, ms.buckets.as<Jac<F>>(), passes);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_msm_vm_merge<F>), dim3(nblk(p.nb, 4 * VM_EPW), p.nwin), dim3(256), vm_lds4<F>(), 0, p, dh.as<uint32_t>(), dso.as<uint32_t>(),
                           dsl.as<Jac<F>>(), max_slots, db.as<Jac<F>>(), passes);
    else
        // engine.hip: hipLaunchKernelGGL(HIP_KERNEL_NAME(k_msm_bucket_merge<F>), dim3(nblk(p.nb, 64), p.nwin), dim3(64), 0, st, p, ms.hist.as<uint32_t>(), ms.slotoffs.as<uint32_t>(),
        //                                ms.slots.as<Jac<F>>(), max_slots, ms.buckets.as<Jac<F>>(), passes, hom);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_msm_bucket_merge<F>), dim3(nblk(p.nb, 64), p.nwin), dim3(64), 0, 0, p, dh.as<uint32_t>(), dso.as<uint32_t>(),
                           dsl.as<Jac<F>>(), max_slots, db.as<Jac<F>>(), passes, hom != 0);
    MS_CHK(hipGetLastError()); MS_CHK(hipDeviceSynchronize());
    MS_CHK(db.get(buckets, (nwb + MS_SLACK) * sizeof(Jac<F>)));
    return 0;
}
template <class F> int segments_(int vm, const MsmPlan& p, const uint32_t* buckets, uint32_t nseg, uint32_t* seg_out) {
    const size_t nwb = (size_t)p.nwin * p.nb, no = (size_t)p.nwin * nseg + MS_SLACK;
    DevBuf db, ds;
    MS_CHK(db.put(buckets, nwb * sizeof(Jac<F>))); MS_CHK(ds.sentinel(no * jw<F>()));
    if (vm)
        // engine.hip: hipLaunchKernelGGL(HIP_KERNEL_NAME(k_msm_vm_segments<F>), dim3(nblk(nseg, 4 * VM_EPW), p.nwin), dim3(256), vm_lds, st, p, ms.buckets.as<Jac<F>>(), cur, nseg);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_msm_vm_segments<F>), dim3(nblk(nseg, 4 * VM_EPW), p.nwin), dim3(256), vm_lds4<F>(), 0, p, db.as<Jac<F>>(), ds.as<Jac<F>>(), nseg);
    else
        // engine.hip: hipLaunchKernelGGL(HIP_KERNEL_NAME(k_msm_segments<F>), dim3(nblk(nseg, 64), p.nwin), dim3(64), 0, st, p, ms.buckets.as<Jac<F>>(), cur, nseg);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_msm_segments<F>), dim3(nblk(nseg, 64), p.nwin), dim3(64), 0, 0, p, db.as<Jac<F>>(), ds.as<Jac<F>>(), nseg);
    MS_CHK(hipGetLastError()); MS_CHK(hipDeviceSynchronize());
    MS_CHK(ds.get(seg_out, no * sizeof(Jac<F>)));
    return 0;
}
template <class F> int reduce_(int vm, const uint32_t* in, uint32_t nin, uint32_t nwin, uint32_t* out, uint32_t nout) {
    const size_t no = (size_t)nwin * nout + MS_SLACK;
    DevBuf di, dout;
    MS_CHK(di.put(in, (size_t)nwin * nin * sizeof(Jac<F>))); MS_CHK(dout.sentinel(no * jw<F>()));
    if (vm)
        // engine.hip: hipLaunchKernelGGL(HIP_KERNEL_NAME(k_msm_vm_reduce<F>), dim3(nblk(nout, 4 * VM_EPW), p.nwin), dim3(256), vm_lds, st, cur, nseg, nxt, nout);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_msm_vm_reduce<F>), dim3(nblk(nout, 4 * VM_EPW), nwin), dim3(256), vm_lds4<F>(), 0, di.as<Jac<F>>(), nin, dout.as<Jac<F>>(), nout);
    else
        // engine.hip: hipLaunchKernelGGL(HIP_KERNEL_NAME(k_msm_seg_reduce<F>), dim3(nblk(nout, 64), p.nwin), dim3(64), 0, st, cur, nseg, nxt, nout);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_msm_seg_reduce<F>), dim3(nblk(nout, 64), nwin), dim3(64), 0, 0, di.as<Jac<F>>(), nin, dout.as<Jac<F>>(), nout);
    MS_CHK(hipGetLastError()); MS_CHK(hipDeviceSynchronize());
    MS_CHK(dout.get(out, no * sizeof(Jac<F>)));
    return 0;
}
template <class F> int finish_(int kind, const MsmPlan& p, const uint32_t* seg, uint32_t nseg, uint32_t* win_out, uint32_t* out) {
    DevBuf ds, dw, dout;
    MS_CHK(ds.put(seg, (size_t)p.nwin * nseg * sizeof(Jac<F>)));
    MS_CHK(dw.sentinel((64 + MS_SLACK) * jw<F>())); MS_CHK(dout.sentinel((1 + MS_SLACK) * jw<F>()));          // engine.hip: ms.win.reserve(64 * sizeof(Jac<F>)), ms.out.reserve(sizeof(Jac<F>))
    if (kind == 0)
        // engine.hip: hipLaunchKernelGGL(HIP_KERNEL_NAME(k_msm_finish_vm<F>), dim3(1), dim3(64), VM_EPW * VmCurve<F>::SLOTS * sizeof(VmSlot), st, p, cur, ms.win.as<Jac<F>>(), ms.out.as<Jac<F>>());
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_msm_finish_vm<F>), dim3(1), dim3(64), vm_lds1<F>(), 0, p, ds.as<Jac<F>>(), dw.as<Jac<F>>(), dout.as<Jac<F>>());
    else
        // engine.hip: hipLaunchKernelGGL(HIP_KERNEL_NAME(k_msm_finish<F>), dim3(1), dim3(64), 0, st, p, cur, nseg, ms.win.as<Jac<F>>(), ms.out.as<Jac<F>>());
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_msm_finish<F>), dim3(1), dim3(64), 0, 0, p, ds.as<Jac<F>>(), nseg, dw.as<Jac<F>>(), dout.as<Jac<F>>());
    MS_CHK(hipGetLastError()); MS_CHK(hipDeviceSynchronize());
    MS_CHK(dw.get(win_out, (64 + MS_SLACK) * sizeof(Jac<F>))); MS_CHK(dout.get(out, (1 + MS_SLACK) * sizeof(Jac<F>)));
    return 0;
}
template <class F> int finish_batch_(const MsmPlan& p, uint32_t rows, const uint32_t* win, uint32_t* out) {
    DevBuf dw, dout;
    MS_CHK(dw.put(win, (size_t)rows * p.nwin * sizeof(Jac<F>))); MS_CHK(dout.sentinel((rows + MS_SLACK) * jw<F>()));
    // engine.hip: hipLaunchKernelGGL(HIP_KERNEL_NAME(k_msm_finish_vm_batch<F>), dim3(nblk(Rc, VM_EPW)), dim3(64), VM_EPW * VmCurve<F>::SLOTS * sizeof(VmSlot), st, p, (uint32_t)Rc, cur, out_dev + r0);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_msm_finish_vm_batch<F>), dim3(nblk(rows, VM_EPW)), dim3(64), vm_lds1<F>(), 0, p, rows, dw.as<Jac<F>>(), dout.as<Jac<F>>());
    MS_CHK(hipGetLastError()); MS_CHK(hipDeviceSynchronize());
    MS_CHK(dout.get(out, (rows + MS_SLACK) * sizeof(Jac<F>)));
    return 0;
}
}  // namespace

// out[0..10): curve, FIX_GRID, MSM_SORT_BLOCK, MSM_SLOT_GROUP, MSM_GROUP_PASSES, MSM_SEG_FAN, VM_EPW, the sentinel, the slack, sizeof(Jac<Fp>)
MS_API void ms_info(uint32_t* out) {
#if defined(RIPP_BLS12_377)
    out[0] = 377;
#else
    out[0] = 381;
#endif
    out[1] = FIX_GRID; out[2] = MSM_SORT_BLOCK; out[3] = MSM_SLOT_GROUP; out[4] = MSM_GROUP_PASSES; out[5] = MSM_SEG_FAN; out[6] = VM_EPW; out[7] = MS_SENTINEL; out[8] = MS_SLACK; out[9] = sizeof(G1J);
}
// the engine's own tile (msm.hpp msm_sort_tile), 0 for a plan the harness refuses
MS_API uint32_t ms_sort_tile(const uint32_t* plan) { const MsmPlan p = plan_of(plan); return plan_ok(p) ? msm_sort_tile(p) : 0u; }

// The counting sort.  digits: nwin x n, every one < nb (checked).  lds != 0: k_msm_hist_lds, k_msm_scan, k_msm_scatter_lds (hist is an output, zeroed over nwin x nb as
// msm_launch does); lds == 0: k_msm_scan and k_msm_scatter on the CALLER's histogram (hist is an input of nwin x nb counts; it must be the digits' own, checked, since the
// scatter's positions are only as good as the runs reserved for them).  Outputs with slack: hist, offs, cursor (after the scatter), slot_offs: nwin x nb + 64 words; spw: nwin + 64; sorted:
// nwin x n + 64.  tiles_out: the grid.x of the two LDS kernels.
MS_API int ms_sort(const uint32_t* plan, const uint16_t* digits, int lds, uint32_t* hist, uint32_t* offs, uint32_t* cursor, uint32_t* slot_offs, uint32_t* spw, uint32_t* sorted, uint32_t* tiles_out) {
    const MsmPlan p = plan_of(plan);
    if (!plan_ok(p)) return -1;
    const size_t n = p.n, nwb = (size_t)p.nwin * p.nb, nd = (size_t)p.nwin * n;
    std::vector<uint32_t> cnt(nwb, 0);
    for (size_t k = 0; k < nd; ++k) { if (digits[k] >= p.nb) return -1; if (digits[k]) ++cnt[(k / n) * p.nb + digits[k]]; }
    if (!lds) for (size_t k = 0; k < nwb; ++k) if (hist[k] != cnt[k]) return -1;
    const uint32_t tile = msm_sort_tile(p);
    if (tile == 0 || tile % MSM_SORT_BLOCK) return -1;
    *tiles_out = nblk(n, tile);
    DevBuf dd, dh, dof, dcu, dso, dsp, dsr;
    MS_CHK(dd.put(digits, nd * 2));
    MS_CHK(dh.sentinel(nwb + MS_SLACK)); MS_CHK(dof.sentinel(nwb + MS_SLACK)); MS_CHK(dcu.sentinel(nwb + MS_SLACK)); MS_CHK(dso.sentinel(nwb + MS_SLACK));
    MS_CHK(dsp.sentinel((size_t)p.nwin + MS_SLACK)); MS_CHK(dsr.sentinel(nd + MS_SLACK));
    if (lds) {
        MS_CHK(hipMemset(dh.p, 0, nwb * 4));                         // engine.hip: HIPCHK(hipMemsetAsync(ms.hist.p, 0, nwb * 4, st));
        // engine.hip: if (lds_sort) hipLaunchKernelGGL(k_msm_hist_lds, dim3(nblk(n, tile), p.nwin), dim3(MSM_SORT_BLOCK), 0, st, ms.digits.as<uint16_t>(), p, tile, ms.hist.as<uint32_t>());
        hipLaunchKernelGGL(k_msm_hist_lds, dim3(nblk(n, tile), p.nwin), dim3(MSM_SORT_BLOCK), 0, 0, dd.as<uint16_t>(), p, tile, dh.as<uint32_t>());
    } else MS_CHK(hipMemcpy(dh.p, hist, nwb * 4, hipMemcpyHostToDevice));
    // engine.hip: hipLaunchKernelGGL(k_msm_scan, dim3(p.nwin), dim3(1024), 0, st, ms.hist.as<uint32_t>(), p, ms.offs.as<uint32_t>(), ms.cursor.as<uint32_t>(), ms.slotoffs.as<uint32_t>(), ms.spw.as<uint32_t>());
    hipLaunchKernelGGL(k_msm_scan, dim3(p.nwin), dim3(1024), 0, 0, dh.as<uint32_t>(), p, dof.as<uint32_t>(), dcu.as<uint32_t>(), dso.as<uint32_t>(), dsp.as<uint32_t>());
    if (lds)
        // engine.hip: if (lds_sort) hipLaunchKernelGGL(k_msm_scatter_lds, dim3(nblk(n, tile), p.nwin), dim3(MSM_SORT_BLOCK), 0, st, ms.digits.as<uint16_t>(), p, tile, ms.cursor.as<uint32_t>(), ms.sorted.as<uint32_t>());
        hipLaunchKernelGGL(k_msm_scatter_lds, dim3(nblk(n, tile), p.nwin), dim3(MSM_SORT_BLOCK), 0, 0, dd.as<uint16_t>(), p, tile, dcu.as<uint32_t>(), dsr.as<uint32_t>());
    else
        // engine.hip: else hipLaunchKernelGGL(k_msm_scatter, dim3(nblk(n, 256)), dim3(256), 0, st, ms.digits.as<uint16_t>(), p, ms.cursor.as<uint32_t>(), ms.sorted.as<uint32_t>());
        hipLaunchKernelGGL(k_msm_scatter, dim3(nblk(n, 256)), dim3(256), 0, 0, dd.as<uint16_t>(), p, dcu.as<uint32_t>(), dsr.as<uint32_t>());
    MS_CHK(hipGetLastError()); MS_CHK(hipDeviceSynchronize());
    MS_CHK(dh.get(hist, (nwb + MS_SLACK) * 4)); MS_CHK(dof.get(offs, (nwb + MS_SLACK) * 4)); MS_CHK(dcu.get(cursor, (nwb + MS_SLACK) * 4)); MS_CHK(dso.get(slot_offs, (nwb + MS_SLACK) * 4));
    MS_CHK(dsp.get(spw, ((size_t)p.nwin + MS_SLACK) * 4)); MS_CHK(dsr.get(sorted, (nd + MS_SLACK) * 4));
    return 0;
}

// One grouping pass, in place.  slots: nwin x max_slots + 64 points (the caller fills the slack with the sentinel), stride: 1, 8 or 64.
MS_API int ms_group(int g2, const uint32_t* plan, const uint32_t* hist, const uint32_t* slot_offs, const uint32_t* spw, uint32_t* slots, uint32_t max_slots, uint32_t stride, int hom) {
    const MsmPlan p = plan_of(plan);
    if (!plan_ok(p) || !layout_ok(p, hist, slot_offs, spw, max_slots) || (stride != 1 && stride != MSM_SLOT_GROUP && stride != MSM_SLOT_GROUP * MSM_SLOT_GROUP)) return -1;
    return g2 ? group_<Fp2>(p, hist, slot_offs, spw, slots, max_slots, stride, hom) : group_<Fp>(p, hist, slot_offs, spw, slots, max_slots, stride, hom);
}
// kind 0: k_msm_vm_merge (homogeneous), 1: k_msm_bucket_merge (hom as given).  slots: nwin x max_slots points.  buckets: nwin x nb + 64 points.
MS_API int ms_merge(int g2, int kind, const uint32_t* plan, const uint32_t* hist, const uint32_t* slot_offs, const uint32_t* spw, const uint32_t* slots, uint32_t max_slots, uint32_t passes, int hom, uint32_t* buckets) {
    const MsmPlan p = plan_of(plan);
    if (!plan_ok(p) || !layout_ok(p, hist, slot_offs, spw, max_slots) || kind < 0 || kind > 1 || passes > (uint32_t)MSM_GROUP_PASSES || (kind == 0 && !hom)) return -1;
    return g2 ? merge_<Fp2>(kind, p, hist, slot_offs, slots, max_slots, passes, hom, buckets) : merge_<Fp>(kind, p, hist, slot_offs, slots, max_slots, passes, hom, buckets);
}
// vm != 0: k_msm_vm_segments (homogeneous), else k_msm_segments (Jacobian).  buckets: nwin x nb points; seg_out: nwin x nseg + 64, nseg = nb / 4 as in msm_launch.
MS_API int ms_segments(int g2, int vm, const uint32_t* plan, const uint32_t* buckets, uint32_t nseg, uint32_t* seg_out) {
    const MsmPlan p = plan_of(plan);
    if (!plan_ok(p) || nseg != (p.nb + p.seg - 1) / p.seg || (size_t)nseg * 4 != p.nb) return -1;       // k_msm_vm_segments reads b[0..4) of every segment
    return g2 ? segments_<Fp2>(vm, p, buckets, nseg, seg_out) : segments_<Fp>(vm, p, buckets, nseg, seg_out);
}
// vm != 0: k_msm_vm_reduce, else k_msm_seg_reduce.  in: nwin x nin points; out: nwin x nout + 64, nout = ceil(nin / MSM_SEG_FAN).
MS_API int ms_reduce(int g2, int vm, const uint32_t* in, uint32_t nin, uint32_t nwin, uint32_t* out, uint32_t nout) {
    if (nin == 0 || nwin == 0 || nwin > MS_MAX_WIN || (size_t)nin * nwin > MS_MAX_ELEMS || nout != (nin + MSM_SEG_FAN - 1) / MSM_SEG_FAN) return -1;
    return g2 ? reduce_<Fp2>(vm, in, nin, nwin, out, nout) : reduce_<Fp>(vm, in, nin, nwin, out, nout);
}
// kind 0: k_msm_finish_vm (seg: nwin homogeneous window sums, nseg == 1), 1: k_msm_finish (seg: nwin x nseg Jacobian sums, nseg <= MSM_SEG_FAN as msm_launch leaves it).
// win_out: 64 + 64 points (the engine's ms.win), out: 1 + 64.  nwin <= 64: the kernels copy one window per lane of their 64.
MS_API int ms_finish(int g2, int kind, const uint32_t* plan, const uint32_t* seg, uint32_t nseg, uint32_t* win_out, uint32_t* out) {
    const MsmPlan p = plan_of(plan);
    if (!plan_ok(p) || p.nwin > 64 || kind < 0 || kind > 1 || nseg == 0 || nseg > (uint32_t)MSM_SEG_FAN || (kind == 0 && nseg != 1)) return -1;
    return g2 ? finish_<Fp2>(kind, p, seg, nseg, win_out, out) : finish_<Fp>(kind, p, seg, nseg, win_out, out);
}
// k_msm_finish_vm_batch.  plan: ONE row's (nwin windows); win: rows x nwin homogeneous window sums; out: rows + 64 Jacobian points.
MS_API int ms_finish_batch(int g2, const uint32_t* plan, uint32_t rows, const uint32_t* win, uint32_t* out) {
    const MsmPlan p = plan_of(plan);
    if (!plan_ok(p) || p.nwin > 64 || rows == 0 || rows > 1024) return -1;
    return g2 ? finish_batch_<Fp2>(p, rows, win, out) : finish_batch_<Fp>(p, rows, win, out);
}
