// TEST INFRASTRUCTURE: the device twin's cases on the CPU (tests/test_device_twin_cases.py).  Before anything is
// asserted about the device, the host compilation alone must show that the cases are worth running: every family's
// verdicts reach both sides, the wide walk's flushes are there and mixed into the groups of 64 consecutive cases a
// wave takes, every sweep table yields the empty and a multi-bit mask, no generator left its domain -- and the host
// compilation agrees with every independent reference.
// Build: g++ -O2 -std=c++17 -ffp-contract=off -march=x86-64-v3 tests/device/twin_host.cpp oracle/pt_oracle.cpp
// usage: twin_host [div]     (every case count divided by div; default 1, the device twin's set)
// Prints one JSON line per family, then one line of the coverage counts; exit 1 on a mismatch.
#include "twin_judge.h"

namespace {

long bad = 0;

template <class F>
twj::Stats run(const std::vector<typename F::Case>& cases, const typename F::Ctx& x, twj::Stats S) {
    const std::vector<uint32_t> words = twj::host_eval<F>(cases, x);
    twj::judge<F>(cases, x, words.data(), nullptr, S);
    return S;
}
void print(const twj::Stats& S) {
    std::printf("{\"family\": \"%s\", \"boolean\": %s, \"has_ref\": %s, \"cases\": %ld, \"positives\": %ld, \"host_vs_ref\": %ld}\n",
                S.family.c_str(), S.boolean ? "true" : "false", S.has_ref ? "true" : "false", S.cases, S.positives, S.vs_ref);
    bad += S.vs_ref;
}
template <class F>
void family(const std::vector<typename F::Case>& cases) {
    print(run<F>(cases, typename F::Ctx(), twj::stats_of<F>()));
}

}  // namespace

int main(int argc, char** argv) {
    const long div = argc > 1 ? std::atol(argv[1]) : 1;
    twf::Cases C;
    twf::generate(C, div < 1 ? 1 : div);

    family<twf::Slab>(C.slab);
    family<twf::SlabWild>(C.slab_wild);
    family<twf::Cull>(C.cull);
    // the sweep: one table at a time; per table, the rays with an empty mask and with more than one bit
    twj::Stats sweep = twj::stats_of<twf::Sweep>();
    long zero[twc::kSweepTables], multi[twc::kSweepTables];
    for (int w = 0; w < twc::kSweepTables; w++) {
        const twc::SweepTable& T = C.sweep[w];
        const twf::SweepCtx x = twf::sweep_ctx(T, T.quads.data(), false);
        const std::vector<uint32_t> words = twj::host_eval<twf::Sweep>(T.rays, x);
        twj::judge<twf::Sweep>(T.rays, x, words.data(), nullptr, sweep);
        zero[w] = multi[w] = 0;
        for (size_t i = 0; i < T.rays.size(); i++) {
            const uint32_t m = words[2 * i];
            zero[w] += m == 0u;
            multi[w] += (m & (m - 1u)) != 0u;
        }
    }
    print(sweep);
    family<twf::Tri>(C.tri);
    family<twf::Aces>(C.aces);
    family<twf::Accum>(C.accum);
    family<twf::Quant>(C.quant);
    family<twf::Target>(C.target);
    family<twf::Retire>(C.retire);
    family<twf::Fold>(C.fold);
    family<twf::WideHits>(C.wide_hits);
    family<twf::WideNext>(C.wide_next);
    family<twf::Rng>(C.rng);
    family<twf::Vec>(C.vec);
    family<twf::Guard>(C.guard);
    family<twf::Sphere>(C.sphere);
    family<twf::LeafChoice>(C.leaf_choice);
    family<twf::Pinhole>(C.pinhole);
    family<twf::SkyDepth>(C.sky_depth);
    family<twf::Bounce>(C.bounce);

    // the lane mix __any exists for: groups of 64 consecutive wide_next cases with a flushing and a non-flushing step
    long mixed = 0, flushes = 0;
    for (size_t g = 0; g + 64 <= C.wide_next.size(); g += 64) {
        int f = 0;
        for (size_t i = g; i < g + 64; i++) f += C.wide_next[i].flush;
        mixed += f > 0 && f < 64;
    }
    for (const twc::WideNextCase& c : C.wide_next) flushes += c.flush;
    std::printf("{\"coverage\": true, \"dropped\": %ld, \"aces_boundaries\": %ld, \"wide_next_flushes\": %ld, \"wide_next_mixed_groups\": %ld, "
                "\"sweep_n\": [%d, %d, %d, %d, %d], \"sweep_zero\": [%ld, %ld, %ld, %ld, %ld], \"sweep_multi\": [%ld, %ld, %ld, %ld, %ld]}\n",
                C.dropped, C.aces_boundaries, flushes, mixed, C.sweep[0].n, C.sweep[1].n, C.sweep[2].n, C.sweep[3].n, C.sweep[4].n, zero[0],
                zero[1], zero[2], zero[3], zero[4], multi[0], multi[1], multi[2], multi[3], multi[4]);
    return bad || C.dropped ? 1 : 0;
}
