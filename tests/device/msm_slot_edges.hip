// Device test harness for the gathered additions of the Pippenger MSM: k_msm_extend_q, k_msm_slot_sum_q and its fix-up kernels k_msm_slot_sum_fix / k_msm_slot_sum_fix_vm
// (ripp_amd/csrc/fq_msm.hpp) and the plain k_msm_slot_sum (msm.hpp).  The other stages are in msm_edges.hip (one translation unit with all of them built several times
// slower than any other harness: the slot-sum kernels of both groups are the largest of the pipeline).  The production headers are included unchanged; every launch uses the
// grid, block and dynamic-LDS expressions of engine.hip (Engine::msm_launch / Engine::msm_batch_dev), quoted at each launch.
//
// Built twice by tests/device/Makefile: libmsm_slot_edges_381.so and libmsm_slot_edges_377.so (-DRIPP_BLS12_377).  Conventions as in msm_edges.hip: HOST arrays in and
// out, the HIP error code returned (-1 = refused arguments, msm_edges_util.hpp), the plan as 8 words, output arrays with MS_SLACK elements of slack behind them.
#include "msm_edges_util.hpp"

using namespace ripp;
using namespace msedge;

static_assert(sizeof(G1A) == 96 && sizeof(G2A) == 192 && sizeof(QAff<Fp>) == 96 && sizeof(QAff<Fp2>) == 192 && sizeof(G1J) == 144 && sizeof(G2J) == 288, "struct sizes the Python side packs");

namespace {
template <class F> constexpr size_t jw() { return sizeof(Jac<F>) / 4; }
template <class F> constexpr size_t vm_lds1() { return VM_EPW * VmCurve<F>::SLOTS * sizeof(VmSlot); }

template <class F> int extend_(const uint32_t* bases, uint32_t n, int split, uint32_t* ext) {
    const size_t no = (size_t)split * n + MS_SLACK;
    DevBuf db, de;
    MS_CHK(db.put(bases, (size_t)n * sizeof(Affine<F>))); MS_CHK(de.sentinel(no * sizeof(Affine<F>) / 4));
    // engine.hip: hipLaunchKernelGGL(HIP_KERNEL_NAME(k_msm_extend_q<F>), dim3(nblk(nreal, 256), split), dim3(256), 0, st, bases, (uint32_t)nreal, split, ms.ext.as<QAff<F>>());
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_msm_extend_q<F>), dim3(nblk(n, 256), split), dim3(256), 0, 0, db.as<Affine<F>>(), n, split, de.as<QAff<F>>());
    MS_CHK(hipGetLastError()); MS_CHK(hipDeviceSynchronize());
    MS_CHK(de.get(ext, no * sizeof(Affine<F>)));
    return 0;
}

template <class F> int slot_sum_(int form, const MsmPlan& p, const uint32_t* bases, const uint32_t* hist, const uint32_t* offs, const uint32_t* slot_offs, const uint32_t* spw,
                                 const uint32_t* sorted, uint32_t max_slots, int hom, uint8_t* flag, uint32_t* slots_mid, uint32_t* slots) {
    const size_t nwb = (size_t)p.nwin * p.nb, ns = (size_t)p.nwin * max_slots, nf = ns + MS_SLACK;
    const int split = (int)(p.n / p.nreal);
    DevBuf db, dh, dof, dso, dsp, dsr, dsl, dfl, dext;
    MS_CHK(db.put(bases, (size_t)p.nreal * sizeof(Affine<F>))); MS_CHK(dh.put(hist, nwb * 4)); MS_CHK(dof.put(offs, nwb * 4)); MS_CHK(dso.put(slot_offs, nwb * 4));
    MS_CHK(dsp.put(spw, (size_t)p.nwin * 4)); MS_CHK(dsr.put(sorted, (size_t)p.nwin * p.n * 4));
    MS_CHK(dsl.put(slots, (ns + MS_SLACK) * sizeof(Jac<F>)));                                    // the caller's buffer: the sentinel, or (fix only) the state before the fix
    MS_CHK(dfl.put(flag, nf));                                                                   // engine.hip: ms.flags.reserve((size_t)p.nwin * max_slots + 16)
    const dim3 grid(nblk(max_slots, 64), p.nwin);
    if (form == 0) {
        // engine.hip: hipLaunchKernelGGL(HIP_KERNEL_NAME(k_msm_slot_sum<F>), dim3(nblk(max_slots, 64), p.nwin), dim3(64), 0, st, bases, p, ms.hist.as<uint32_t>(), ms.offs.as<uint32_t>(),
        //                                ms.slotoffs.as<uint32_t>(), ms.spw.as<uint32_t>(), ms.sorted.as<uint32_t>(), ms.slots.as<Jac<F>>(), max_slots, hom);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_msm_slot_sum<F>), grid, dim3(64), 0, 0, db.as<Affine<F>>(), p, dh.as<uint32_t>(), dof.as<uint32_t>(), dso.as<uint32_t>(), dsp.as<uint32_t>(),
                           dsr.as<uint32_t>(), dsl.as<Jac<F>>(), max_slots, hom != 0);
    } else if (form == 1 || form == 2) {
        MS_CHK(dext.sentinel(((size_t)p.n + MS_SLACK) * sizeof(Affine<F>) / 4));
        // engine.hip: hipLaunchKernelGGL(HIP_KERNEL_NAME(k_msm_extend_q<F>), dim3(nblk(nreal, 256), split), dim3(256), 0, st, bases, (uint32_t)nreal, split, ms.ext.as<QAff<F>>());
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_msm_extend_q<F>), dim3(nblk(p.nreal, 256), split), dim3(256), 0, 0, db.as<Affine<F>>(), p.nreal, split, dext.as<QAff<F>>());
        // engine.hip: hipLaunchKernelGGL(HIP_KERNEL_NAME(k_msm_slot_sum_q<F>), dim3(nblk(max_slots, 64), p.nwin), dim3(64), 0, st, ms.ext.as<QAff<F>>(), p, ms.hist.as<uint32_t>(), ms.offs.as<uint32_t>(),
        //                                ms.slotoffs.as<uint32_t>(), ms.spw.as<uint32_t>(), ms.sorted.as<uint32_t>(), ms.slots.as<Jac<F>>(), max_slots, hom, ms.flags.as<uint8_t>());
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_msm_slot_sum_q<F>), grid, dim3(64), 0, 0, dext.as<QAff<F>>(), p, dh.as<uint32_t>(), dof.as<uint32_t>(), dso.as<uint32_t>(), dsp.as<uint32_t>(),
                           dsr.as<uint32_t>(), dsl.as<Jac<F>>(), max_slots, hom != 0, dfl.as<uint8_t>());
    }
    MS_CHK(hipGetLastError()); MS_CHK(hipDeviceSynchronize());
    MS_CHK(dsl.get(slots_mid, (ns + MS_SLACK) * sizeof(Jac<F>)));                                 // after the throughput kernel (fix only: the caller's state)
    if (form == 1 || form == 3)
        // engine.hip: hipLaunchKernelGGL(HIP_KERNEL_NAME(k_msm_slot_sum_fix<F>), dim3(FIX_GRID), dim3(64), 0, st, bases, p, ms.hist.as<uint32_t>(), ms.offs.as<uint32_t>(),
        //                                ms.slotoffs.as<uint32_t>(), ms.spw.as<uint32_t>(), ms.sorted.as<uint32_t>(), ms.slots.as<Jac<F>>(), max_slots, hom, ms.flags.as<uint8_t>());
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_msm_slot_sum_fix<F>), dim3(FIX_GRID), dim3(64), 0, 0, db.as<Affine<F>>(), p, dh.as<uint32_t>(), dof.as<uint32_t>(), dso.as<uint32_t>(), dsp.as<uint32_t>(),
                           dsr.as<uint32_t>(), dsl.as<Jac<F>>(), max_slots, hom != 0, dfl.as<uint8_t>());
    else if (form == 2 || form == 4)
        // engine.hip: hipLaunchKernelGGL(HIP_KERNEL_NAME(k_msm_slot_sum_fix_vm<F>), dim3(FIX_GRID), dim3(64), VM_EPW * VmCurve<F>::SLOTS * sizeof(VmSlot), st, bases, p, ms.hist.as<uint32_t>(), ms.offs.as<uint32_t>(),
        //                                ms.slotoffs.as<uint32_t>(), ms.spw.as<uint32_t>(), ms.sorted.as<uint32_t>(), ms.slots.as<Jac<F>>(), max_slots, ms.flags.as<uint8_t>(), trace_on() ? ms.nflag.as<uint32_t>() : nullptr);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_msm_slot_sum_fix_vm<F>), dim3(FIX_GRID), dim3(64), vm_lds1<F>(), 0, db.as<Affine<F>>(), p, dh.as<uint32_t>(), dof.as<uint32_t>(), dso.as<uint32_t>(), dsp.as<uint32_t>(),
                           dsr.as<uint32_t>(), dsl.as<Jac<F>>(), max_slots, dfl.as<uint8_t>(), (uint32_t*)nullptr);
    MS_CHK(hipGetLastError()); MS_CHK(hipDeviceSynchronize());
    MS_CHK(dsl.get(slots, (ns + MS_SLACK) * sizeof(Jac<F>))); MS_CHK(dfl.get(flag, nf));
    return 0;
}
}  // namespace

MS_API void mss_info(uint32_t* out) {
#if defined(RIPP_BLS12_377)
    out[0] = 377;
#else
    out[0] = 381;
#endif
    out[1] = FIX_GRID; out[2] = MS_SENTINEL; out[3] = MS_SLACK; out[4] = VM_EPW;
}
// bases: n affine points (Montgomery-384, (0, 0) = identity); ext: split x n + 64 entries of the same size.  split: 1 or 2 (G1), 1 or 4 (G2).
MS_API int mss_extend(int g2, const uint32_t* bases, uint32_t n, int split, uint32_t* ext) {
    if (n == 0 || n > MS_MAX_N || !(split == 1 || split == (g2 ? 4 : 2))) return -1;
    return g2 ? extend_<Fp2>(bases, n, split, ext) : extend_<Fp>(bases, n, split, ext);
}
// form 0: k_msm_slot_sum; 1: k_msm_extend_q, k_msm_slot_sum_q, k_msm_slot_sum_fix; 2: the same with k_msm_slot_sum_fix_vm (hom only, as in msm_launch);
// 3 / 4: the fix-up kernel alone (k_msm_slot_sum_fix / _fix_vm) over the caller's flags and slot sums.
// flag: nwin x max_slots + 64 bytes, in and out (the caller's bytes are what a reused buffer holds).  slots: nwin x max_slots + 64 points, in and out; slots_mid: the same
// array as it is after the first launch.  The layout arrays are the caller's, verified here (layout_ok, runs_ok): a test decides which terms share a slot and in which order.
MS_API int mss_slot_sum(int g2, int form, const uint32_t* plan, const uint32_t* bases, const uint32_t* hist, const uint32_t* offs, const uint32_t* slot_offs, const uint32_t* spw,
                        const uint32_t* sorted, uint32_t max_slots, int hom, uint8_t* flag, uint32_t* slots_mid, uint32_t* slots) {
    const MsmPlan p = plan_of(plan);
    const int split = plan_ok(p) ? (int)(p.n / p.nreal) : 0;
    if (!plan_ok(p) || form < 0 || form > 4 || !(split == 1 || split == (g2 ? 4 : 2)) || !layout_ok(p, hist, slot_offs, spw, max_slots) || !runs_ok(p, hist, offs, sorted)) return -1;
    if ((form == 2 || form == 4) && !hom) return -1;
    return g2 ? slot_sum_<Fp2>(form, p, bases, hist, offs, slot_offs, spw, sorted, max_slots, hom, flag, slots_mid, slots)
              : slot_sum_<Fp>(form, p, bases, hist, offs, slot_offs, spw, sorted, max_slots, hom, flag, slots_mid, slots);
}
