// TEST INFRASTRUCTURE: the comparer of the device twin -- word for word, no tolerance.  Host code only.
#pragma once

#include "twin_families.h"

#include <string>

namespace twj {

struct Stats {
    std::string family;
    bool boolean = false, has_ref = false;
    long cases = 0, positives = 0, vs_host = 0, vs_ref = 0;
};
template <class F>
Stats stats_of() {
    Stats S;
    S.family = F::name();
    S.boolean = F::boolean;
    S.has_ref = F::has_ref;
    return S;
}

inline long shown = 0;   // the first 10 mismatches of the run are printed
template <class F>
void report(const char* what, const typename F::Case& c, const uint32_t* got, const uint32_t* want) {
    if (shown++ >= 10) return;
    std::fprintf(stderr, "%s %s: ", F::name(), what);
    F::show(c);
    std::fprintf(stderr, ": got");
    for (int w = 0; w < F::W; w++) std::fprintf(stderr, " %08x", got[w]);
    std::fprintf(stderr, ", want");
    for (int w = 0; w < F::W; w++) std::fprintf(stderr, " %08x", want[w]);
    std::fprintf(stderr, "\n");
}

// the host compilation's words of every case
template <class F>
std::vector<uint32_t> host_eval(const std::vector<typename F::Case>& cases, const typename F::Ctx& x) {
    std::vector<uint32_t> out(cases.size() * (size_t)F::W);
    for (size_t i = 0; i < cases.size(); i++) F::eval(cases[i], x, &out[i * F::W]);
    return out;
}

// `got`: the words under judgement, W per case.  `host`: the host compilation's words of the same cases, or null
// when `got` is the host's own.  x: the context with host pointers.
template <class F>
void judge(const std::vector<typename F::Case>& cases, const typename F::Ctx& x, const uint32_t* got, const uint32_t* host, Stats& S) {
    for (size_t i = 0; i < cases.size(); i++) {
        const uint32_t* g = got + i * F::W;
        S.cases++;
        S.positives += F::positive(cases[i], host ? host + i * F::W : g);
        if (host) {
            const uint32_t* h = host + i * F::W;
            bool bad = false;
            for (int w = 0; w < F::W; w++) bad = bad || g[w] != h[w];
            if (bad) { S.vs_host++; report<F>("device != host", cases[i], g, h); }
        }
        uint32_t r[F::W];
        F::ref(cases[i], x, g, r);
        bool bad = false;
        for (int w = 0; w < F::W; w++) bad = bad || g[w] != r[w];
        if (bad) { S.vs_ref++; report<F>("!= reference", cases[i], g, r); }
    }
}

}  // namespace twj
