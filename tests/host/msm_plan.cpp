// Stand-alone driver of the host side of the Pippenger plan: msm_tune_ok, msm_plan (ripp_amd/csrc/msm.hpp) and msm_plan_batch (msm_batch.hpp), compiled for the
// host only (tests/test_msm_plan_cpu.py builds and runs it; no device, no library, no kernel is launched).
//
// stdin, one request per line, decimal:   <nreal> <split> <rows> <c> <ch> <gmin>        rows == 0: msm_plan, otherwise msm_plan_batch over `rows` rows
// stdout, one line per request:           <ok> <c> <nwin> <nb> <n> <ch> <seg> <nreal> <gmin> <tile>
//   ok = msm_tune_ok of the tuning members; when it is 0 the plan is NOT formed (the engine refuses such a call) and the other fields are printed as 0.
//   tile = msm_sort_tile of the plan (for rows > 0: of the batch's rows * nwin virtual windows, as msm_batch_dev forms it).
#include "msm_batch.hpp"
#include <cstdio>

using namespace ripp;

int main() {
    unsigned long long nreal, rows; int split; long long c; unsigned long long ch, gmin;
    while (scanf("%llu %d %llu %lld %llu %llu", &nreal, &split, &rows, &c, &ch, &gmin) == 6) {
        MsmTune t; t.c = (int)c; t.ch = (uint32_t)ch; t.gmin = (uint32_t)gmin;
        if (!msm_tune_ok(t)) { printf("0 0 0 0 0 0 0 0 0 0\n"); continue; }
        const MsmPlan p = rows ? msm_plan_batch((size_t)nreal, split, (size_t)rows, t) : msm_plan((size_t)nreal, split, t);
        MsmPlan pb = p; if (rows) pb.nwin = (int)(rows * (unsigned long long)p.nwin);
        printf("1 %d %d %u %u %u %u %u %u %u\n", p.c, p.nwin, p.nb, p.n, p.ch, p.seg, p.nreal, p.gmin, msm_sort_tile(pb));
    }
    return 0;
}
