// Replays the launch plan of a two-group fused stretch (csrc/step_schedule.h: StepPlanner) against a model of every buffer the fused
// step reads and writes, for tests/test_step_hazards.py (plain C++: no HIP, no library).
//
// The model (dev_step_impl.h, RunCall::run_fused).  Launch i of a stretch over the chains R, with q = parity of i, p = q ^ 1, A(i) the
// swap pair of iteration i:
//   writes, for m in R:   P[q][m]     the chain's state of parity q, slot, prop_logPr, prop_st, quick, part, psum (commit_chain, the tiles)
//                         N[(i+1)%3][m]  the chain's two candidate slots 2m, 2m+1 of iteration i+1 (every array of the candidate set)
//                         LZ[q][m]    L z of iteration i+2
//                         X[(i+1)%3][block of m][half]  for the two chains of A(i): the pair's cross candidates, slots 2C + 4 block + 2 half
//                                     + {0, 1}; block = (m >= xsplit), half = 0 for the pair's first chain, 1 for its second
//   reads, for every c in K = R + the partners of R in A(i) (cross candidates are built on the partner's vectors) + the partners of
//   those in A(i-1) (deciding iteration i-1 for a chain of that pair needs both chains' sums):
//                         P[p][c], N[i%3][c], N[(i-1)%3][c] (the proposal of i, the accepted proposal of i-1),
//                         X[i%3][block of c][half] when c is in A(i-1), X[(i-1)%3][block of c][half] when c is in A(i-2)
//                         (where the chain's proposal of iteration i / i-1 lives after a swap)
//                         and LZ[p][m] for m in R (L z of iteration i+1, for the candidates).
//   The first launch of a stretch (settled chains) reads P[q][m], N[i%3][m], LZ[p][m] of its own chains only.  The closing launches
//   (commit workgroups alone, iteration = one past the last) read like a launch without a pair of its own and write P[q][m].
//   The records go to rows of their own (iteration, chain); the counters are atomic.  Everything before the stretch is complete.
// Two launches are ordered through the same stream or through a planned wait (an event recorded on one stream, waited for by the other:
// everything enqueued on the first before the record precedes everything enqueued on the second after the wait).
// A hazard: a read or a write of an item whose last writer is not ordered before it, or a write not ordered after a reader of the item.
//
//   step_hazard_driver <seed>
//   step_hazard_driver pairs <C> <n> <seed0> <count>      (for tests/test_gpu_straddle_window.py, which picks a seed by what its draws hold)
// Output lines:
//   A <seed> <pair of iteration 0> ... <of iteration n-1>     dN_mixing = 1, seeds seed0 .. seed0 + count - 1
//   H <C> <xsplit> <what> <mode> <sequences> <hazards> <unsplit pairs> <windows> <joints> <first hazard or ->
//      what: x4 = every pair sequence of length 4 (pairs -1 .. C-2), x6 = every sequence of length 6 (7 and 8 chains, mode 0),
//            r = random sequences of length 48
//      mode: 0 the plan as it is; 1 without the wait of s1 for st after a window; 2 without the wait of st for s1 before a window;
//            3 / 4 without the waits inside a window of s1 for st / of st for s1
//   W <C> <xsplit> <k> <A> <b> <window> <st_waits_s1> <s1_waits_st>     the plan itself over one random sequence (last line: the closing launches)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../tamcmc-c_amd/csrc/rng.h"
#include "../tamcmc-c_amd/csrc/step_schedule.h"

using namespace tamcmc;

namespace {

struct Stamp { int stream, seq; };                 // a launch: the seq-th of its stream
struct Clock { int seen[2]; };                     // launches of each stream known to precede

struct Item {
    Stamp writer{-1, 0};
    int reader[2] = {0, 0};  // the last reader of each stream since the last write (a stream's launches are ordered among themselves)
};

constexpr int MAXC = 20;

struct Model {
    int C, xs;
    Item items[7 * MAXC + 12];
    Clock clk[2];      // per stream: what its next launch follows
    int n[2];          // launches enqueued per stream
    long hazards = 0;
    std::string first_hazard;

    Model(int C_, int xs_) : C(C_), xs(xs_) { clk[0] = clk[1] = Clock{{0, 0}}; n[0] = n[1] = 0; }
    int iP(int par, int c) const { return par * C + c; }
    int iLZ(int par, int c) const { return 2 * C + par * C + c; }
    int iN(int set, int c) const { return 4 * C + set * C + c; }
    int iX(int set, int c, int half) const { return 7 * C + (set * 2 + (c >= xs ? 1 : 0)) * 2 + half; }

    static bool before(const Stamp &w, const Clock &k) { return w.stream < 0 || k.seen[w.stream] >= w.seq; }
    void hazard(const char *kind, int item, long i) {
        if (!hazards) first_hazard = std::string(kind) + ":" + std::to_string(item) + "@" + std::to_string(i);
        hazards++;
    }
    void read(int item, const Stamp &me, const Clock &k, long i) {
        Item &t = items[(size_t)item];
        if (!before(t.writer, k)) hazard("raw", item, i);
        if (me.seq > t.reader[me.stream]) t.reader[me.stream] = me.seq;
    }
    void write(int item, const Stamp &me, const Clock &k, long i) {
        Item &t = items[(size_t)item];
        if (!before(t.writer, k)) hazard("waw", item, i);
        for (int s = 0; s < 2; s++)
            if (s != me.stream && t.reader[s] > k.seen[s]) { hazard("war", item, i); break; }
        t.writer = me;
        t.reader[0] = t.reader[1] = 0;
    }
    // `to` waits for an event recorded now on `from`
    void wait(int to, int from) {
        for (int s = 0; s < 2; s++)
            if (clk[from].seen[s] > clk[to].seen[s]) clk[to].seen[s] = clk[from].seen[s];
    }

    static bool in_pair(int c, int A) { return A >= 0 && (c == A || c == A + 1); }
    static int partner(int c, int A) { return c == A ? A + 1 : A; }

    // launch i over [lo, hi) on `stream`; A0 / A1 / A2: the pairs of iterations i, i-1, i-2 (-1: none, or before the stretch)
    void launch(int stream, int lo, int hi, long i, bool first, bool close, int A0, int A1, int A2) {
        if (lo >= hi) return;
        const Stamp me{stream, ++n[stream]};
        const Clock k = clk[stream];
        const int q = (int)(i & 1), p = q ^ 1;
        const int e0 = (int)(i % 3), em = (int)((i + 2) % 3), ep = (int)((i + 1) % 3);
        unsigned K = 0;  // (bit c: chain c)
        for (int m = lo; m < hi; m++) K |= 1u << m;
        if (!first) {
            if (!close)
                for (int m = lo; m < hi; m++)
                    if (in_pair(m, A0)) K |= 1u << partner(m, A0);
            unsigned K2 = K;
            for (int c = 0; c < C; c++)
                if ((K >> c & 1u) && in_pair(c, A1)) K2 |= 1u << partner(c, A1);
            K = K2;
        }
        for (int c = 0; c < C; c++) {
            if (!(K >> c & 1u)) continue;
            if (first) {
                read(iP(q, c), me, k, i);
                read(iN(e0, c), me, k, i);
            } else {
                read(iP(p, c), me, k, i);
                read(iN(e0, c), me, k, i);
                read(iN(em, c), me, k, i);
                if (in_pair(c, A1)) read(iX(e0, c, c == A1 ? 0 : 1), me, k, i);
                if (in_pair(c, A2)) read(iX(em, c, c == A2 ? 0 : 1), me, k, i);
            }
        }
        if (!close)
            for (int m = lo; m < hi; m++) read(iLZ(p, m), me, k, i);
        for (int m = lo; m < hi; m++) {
            write(iP(q, m), me, k, i);
            if (close) continue;
            write(iN(ep, m), me, k, i);
            write(iLZ(q, m), me, k, i);
        }
        if (!close && A0 >= lo && A0 + 1 < hi) {
            write(iX(ep, A0, 0), me, k, i);
            write(iX(ep, A0 + 1, 1), me, k, i);
        }
        clk[stream].seen[stream] = me.seq;  // (later launches of the stream follow this one)
    }
};

struct Tally { long seqs = 0, hazards = 0, unsplit = 0, windows = 0, joints = 0; std::string first; };

// One stretch over the pairs seq[0 .. n), then its closing launches.
void run_stretch(int C, int xs, const int *seq, int n, int mode, Tally &t, bool print) {
    Model M(C, xs);
    StepPlanner pl(true, C, xs);
    bool prev_window = false;
    for (int k = 0; k <= n; k++) {
        const bool close = k == n;
        const int A0 = close ? -1 : seq[k], A1 = k >= 1 ? seq[k - 1] : -1, A2 = k >= 2 ? seq[k - 2] : -1;
        StepPlan p = pl.next(A0);
        if (print) printf("W %d %d %d %d %d %d %d %d\n", C, xs, k, A0, p.b, p.window ? 1 : 0, p.st_waits_s1 ? 1 : 0, p.s1_waits_st ? 1 : 0);
        bool st_w = p.st_waits_s1, s1_w = p.s1_waits_st;
        if (mode == 1 && prev_window && !p.window && p.b == xs) s1_w = false;
        if (mode == 2 && p.window && !prev_window) st_w = false;
        if (mode == 3 && p.window && prev_window) s1_w = false;
        if (mode == 4 && p.window && prev_window) st_w = false;
        if (st_w) M.wait(0, 1);
        if (s1_w) M.wait(1, 0);
        // every pair this iteration needs lies inside one launch
        for (int A : {A0, k >= 1 ? A1 : -1})
            if (A >= 0 && A < p.b && A + 1 >= p.b && p.b < C) t.unsplit++;
        if (p.b <= 0 || p.b > C) t.unsplit++;
        M.launch(0, 0, p.b, k, k == 0, close, A0, A1, A2);
        M.launch(1, p.b, C, k, k == 0, close, A0, A1, A2);
        if (!close) { t.windows += p.window ? 1 : 0; t.joints += p.b == C ? 1 : 0; }
        prev_window = p.window;
    }
    t.seqs++;
    if (M.hazards && !t.hazards) {
        t.first = M.first_hazard + "/";
        for (int k = 0; k < n; k++) t.first += (k ? "," : "") + std::to_string(seq[k]);
    }
    t.hazards += M.hazards;
}

void exhaustive(int C, int xs, int len, int mode, Tally &t) {
    std::vector<int> seq((size_t)len, -1);
    for (;;) {
        run_stretch(C, xs, seq.data(), len, mode, t, false);
        int k = 0;
        while (k < len && ++seq[(size_t)k] > C - 2) seq[(size_t)k++] = -1;
        if (k == len) break;
    }
}

// pairs drawn near the boundary half of the time: windows, repeated straddles and the joint fallback in every few iterations
void random_seq(uint64_t seed, uint64_t n, int C, int xs, int *seq, int len) {
    for (int k = 0; k < len; k++) {
        double u, u2;
        rng_uniform2(seed, RNG_SWAP, (uint32_t)C, n, (uint32_t)k, u, u2);
        int A = u < 0.5 ? xs - 2 + (int)(u2 * 4.0) : -1 + (int)(u2 * (double)C);
        if (A > C - 2) A = C - 2;
        if (A < -1) A = -1;
        seq[k] = A;
    }
}

}  // namespace

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    if (std::string(argv[1]) == "pairs") {
        if (argc < 6) return 2;
        const int C = atoi(argv[2]);
        const long n = atol(argv[3]);
        const uint64_t seed0 = strtoull(argv[4], nullptr, 10), count = strtoull(argv[5], nullptr, 10);
        for (uint64_t sd = seed0; sd < seed0 + count; sd++) {
            printf("A %llu", (unsigned long long)sd);
            for (long it = 0; it < n; it++) printf(" %d", swap_pair(sd, C, 1, it, nullptr));
            printf("\n");
        }
        return 0;
    }
    const uint64_t seed = strtoull(argv[1], nullptr, 10);
    const int Cs[4] = {7, 8, 9, MAXC};
    for (int C : Cs)
        for (int xs : {C / 2, C / 2 + 1})
            for (int mode = 0; mode < 5; mode++) {
                if (C <= 9 || mode <= 1) {
                    Tally t;
                    exhaustive(C, xs, 4, mode, t);
                    printf("H %d %d x4 %d %ld %ld %ld %ld %ld %s\n", C, xs, mode, t.seqs, t.hazards, t.unsplit, t.windows, t.joints, t.hazards ? t.first.c_str() : "-");
                }
                if (C <= 8 && mode == 0) {
                    Tally t;
                    exhaustive(C, xs, 6, mode, t);
                    printf("H %d %d x6 %d %ld %ld %ld %ld %ld %s\n", C, xs, mode, t.seqs, t.hazards, t.unsplit, t.windows, t.joints, t.hazards ? t.first.c_str() : "-");
                }
                {
                    Tally t;
                    int seq[48];
                    for (uint64_t n = 0; n < (mode ? 2000u : 10000u); n++) {
                        random_seq(seed, n, C, xs, seq, 48);
                        run_stretch(C, xs, seq, 48, mode, t, false);
                    }
                    printf("H %d %d r %d %ld %ld %ld %ld %ld %s\n", C, xs, mode, t.seqs, t.hazards, t.unsplit, t.windows, t.joints, t.hazards ? t.first.c_str() : "-");
                }
            }
    for (int C : {8, 20}) {
        Tally t;
        int seq[48];
        random_seq(seed, 12345, C, C / 2, seq, 48);
        run_stretch(C, C / 2, seq, 48, 0, t, true);
    }
    return 0;
}
