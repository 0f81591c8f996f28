// Replays the launch plan of a two-group fused stretch (csrc/step_schedule.h: StepPlanner) against a model of the tiles' per-chain
// accumulators (FusedArgs::qacc, dev_step_impl.h), for tests/test_qacc_protocol.py (plain C++: no HIP, no library).
//
// The model.  One item per (chain, set), set = iteration mod 3.  Launch i of a stretch over the chains R, A(i) the swap pair of iteration i:
//   adds   (c, i mod 3)       for c in R: the likelihood tiles of chain c (StepTiles::store_sums) -- not in a closing launch
//   reads  (c, (i-1) mod 3)   not in the first launch of a stretch (settled chains).  By chain m's tiles and commit workgroup: c = m and,
//                             when m is in A(i-1), its partner (the shortcut sums both chains of the pair); by the cross candidates'
//                             roles of a chain m of A(i), which decide iteration i-1 for m's partner s in A(i): c = s and, when s is in
//                             A(i-1), its partner there
//   zeroes (m, (i+1) mod 3)   for m in R: chain m's commit workgroup
// The closing launches (iteration = one past the last, commit workgroups alone): a chain outside A(i-1) reads (m, (i-1) mod 3) and then
// zeroes its three sets; the FIRST chain of A(i-1) reads both chains' items and then zeroes both chains' three sets; the second chain
// does neither.  Before the first stretch every item is zero (the allocation).
// Two launches are ordered through the same stream or through a planned wait, as in tests/step_hazard_driver.cpp; inside one launch
// nothing is ordered except what ONE workgroup does, in program order.
// What is checked, per item, as the operations arrive (the launches of an iteration after those of the iteration before, which is
// one of the orders the plan allows):
//   * every zero since the item was last in use happens before every add of the next launch that adds;
//   * an add never lands on an item that has been read since its last zero (a zero is missing), nor on another launch's adds;
//   * every add happens before every read (by the next launch), and every add and read before the next zero;
//   * after the closing launches every item is zero again.
//
//   qacc_protocol_driver <seed>
// Output lines:
//   Q <C> <xsplit> <what> <mode> <sequences> <violations> <first violation or ->
//      what: x4 = every sequence of four pairs (-1 .. C-2) and the closing launches, the stretch starting at iteration 0;
//            two = random sequences: a stretch of 3, 4 or 5 pairs starting at iteration 0, 1 or 2, the streams idle after its closing
//                  launches (the end of a run() call), then a second stretch of four pairs that starts armed where the first ended
//      mode: 0 the protocol as it is; 1 without the commit workgroups' zero; 2 without the closing launches' zeroes
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../tamcmc-c_amd/csrc/rng.h"
#include "../tamcmc-c_amd/csrc/step_schedule.h"

using namespace tamcmc;

namespace {

struct Clock { int seen[2]; };  // launches of each stream known to precede
struct Op {
    int stream, seq;   // the launch: the seq-th of its stream
    Clock clk;         // what that launch follows
    int wg, ord;       // the workgroup inside the launch and the operation's place in its program
    long it;           // the launch's iteration
};

// does X happen before Y?
bool hb(const Op &x, const Op &y) {
    if (x.stream == y.stream && x.seq == y.seq) return x.wg == y.wg && x.ord < y.ord;
    return y.clk.seen[x.stream] >= x.seq;
}

struct Item {
    std::vector<Op> zeros, adds, reads;  // since the item was last zeroed after use (zeros: since then)
};

constexpr int MAXC = 20;
enum { WG_TILES = 0, WG_COMMIT = 1, WG_ROLES = 2 };

struct Model {
    int C, xs, mode;
    Item items[3 * MAXC];
    Clock clk[2];
    int n[2];
    long violations = 0;
    std::string first;

    Model(int C_, int xs_, int mode_) : C(C_), xs(xs_), mode(mode_) { clk[0] = clk[1] = Clock{{0, 0}}; n[0] = n[1] = 0; }
    Item &at(int c, long it) { return items[(size_t)(((it % 3) + 3) % 3) * MAXC + c]; }
    void bad(const char *kind, int c, long it) {
        if (!violations) first = std::string(kind) + ":" + std::to_string(c) + "@" + std::to_string(it);
        violations++;
    }
    void add(int c, const Op &op) {
        Item &t = at(c, op.it);
        if (!t.reads.empty()) bad("add-on-read-item", c, op.it);
        for (const Op &a : t.adds)
            if (a.it != op.it) { bad("add-on-adds", c, op.it); break; }
        for (const Op &z : t.zeros)
            if (!hb(z, op)) { bad("zero-not-before-add", c, op.it); break; }
        t.adds.push_back(op);
    }
    void read(int c, long set_it, const Op &op) {
        Item &t = at(c, set_it);
        for (const Op &a : t.adds) {
            if (a.it != set_it) { bad("read-of-other-adds", c, op.it); break; }
            if (!hb(a, op)) { bad("add-not-before-read", c, op.it); break; }
        }
        for (const Op &z : t.zeros)
            if (!hb(z, op)) { bad("zero-not-before-read", c, op.it); break; }
        t.reads.push_back(op);
    }
    void zero(int c, long set_it, const Op &op) {
        Item &t = at(c, set_it);
        for (const Op &a : t.adds)
            if (!hb(a, op)) { bad("add-not-before-zero", c, op.it); break; }
        for (const Op &r : t.reads)
            if (!hb(r, op)) { bad("read-not-before-zero", c, op.it); break; }
        if (!t.adds.empty() || !t.reads.empty()) t.zeros.clear();
        t.adds.clear();
        t.reads.clear();
        t.zeros.push_back(op);
    }
    void wait(int to, int from) {
        for (int s = 0; s < 2; s++)
            if (clk[from].seen[s] > clk[to].seen[s]) clk[to].seen[s] = clk[from].seen[s];
    }
    void idle() { wait(0, 1); wait(1, 0); }  // the host has waited for both streams
    void all_zero(long it) {
        for (int e = 0; e < 3; e++)
            for (int c = 0; c < C; c++)
                if (!items[(size_t)e * MAXC + c].adds.empty() || !items[(size_t)e * MAXC + c].reads.empty()) bad("left-in-use", c, it);
    }

    static bool in_pair(int c, int A) { return A >= 0 && (c == A || c == A + 1); }
    static int partner(int c, int A) { return c == A ? A + 1 : A; }

    // launch of iteration `it` over [lo, hi) on `stream`; A0 / A1: the pairs of iterations it and it-1 (-1: none, or before the stretch)
    void launch(int stream, int lo, int hi, long it, bool first_, bool close, int A0, int A1) {
        if (lo >= hi) return;
        Op me{stream, ++n[stream], clk[stream], 0, 0, it};
        auto op = [&](int kind, int m, int ord) { Op o = me; o.wg = 3 * m + kind; o.ord = ord; return o; };
        for (int m = lo; m < hi; m++) {
            if (close) {
                if (in_pair(m, A1) && m != A1) continue;  // the pair's second chain: its first chain's workgroup
                const int cnt = in_pair(m, A1) ? 2 : 1;
                for (int c = m; c < m + cnt; c++) read(c, it - 1, op(WG_COMMIT, m, 0));
                if (mode != 2)
                    for (int c = m; c < m + cnt; c++)
                        for (int e = 0; e < 3; e++) zero(c, it + e, op(WG_COMMIT, m, 1));
                continue;
            }
            if (!first_) {
                for (int kind : {WG_TILES, WG_COMMIT}) {
                    read(m, it - 1, op(kind, m, 0));
                    if (in_pair(m, A1)) read(partner(m, A1), it - 1, op(kind, m, 0));
                }
                if (in_pair(m, A0)) {
                    const int s = partner(m, A0);
                    read(s, it - 1, op(WG_ROLES, m, 0));
                    if (in_pair(s, A1)) read(partner(s, A1), it - 1, op(WG_ROLES, m, 0));
                }
            }
            add(m, op(WG_TILES, m, 1));
            if (mode != 1) zero(m, it + 1, op(WG_COMMIT, m, 1));
        }
        clk[stream].seen[stream] = me.seq;
    }
};

struct Tally { long seqs = 0, violations = 0; std::string first; };

// One stretch over the pairs seq[0 .. n) from iteration it0 on, then its closing launches.
void run_stretch(Model &M, StepPlanner &pl, long it0, const int *seq, int n) {
    for (int k = 0; k <= n; k++) {
        const bool close = k == n;
        const int A0 = close ? -1 : seq[k], A1 = k >= 1 ? seq[k - 1] : -1;
        const StepPlan p = pl.next(A0);
        if (p.st_waits_s1) M.wait(0, 1);
        if (p.s1_waits_st) M.wait(1, 0);
        M.launch(0, 0, p.b, it0 + k, k == 0, close, A0, A1);
        M.launch(1, p.b, M.C, it0 + k, k == 0, close, A0, A1);
    }
    M.all_zero(it0 + n);
}

void tally(Tally &t, const Model &M, const int *seq, int n) {
    t.seqs++;
    if (M.violations && !t.violations) {
        t.first = M.first + "/";
        for (int k = 0; k < n; k++) t.first += (k ? "," : "") + std::to_string(seq[k]);
    }
    t.violations += M.violations;
}

void exhaustive(int C, int xs, int len, int mode, Tally &t) {
    std::vector<int> seq((size_t)len, -1);
    for (;;) {
        Model M(C, xs, mode);
        StepPlanner pl(true, C, xs);
        run_stretch(M, pl, 0, seq.data(), len);
        tally(t, M, seq.data(), len);
        int k = 0;
        while (k < len && ++seq[(size_t)k] > C - 2) seq[(size_t)k++] = -1;
        if (k == len) break;
    }
}

// pairs drawn near the boundary half of the time, as in tests/step_hazard_driver.cpp
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

void two_stretches(uint64_t seed, int C, int xs, int mode, Tally &t) {
    int seq[9];
    for (uint64_t n = 0; n < 3000; n++) {
        random_seq(seed, n, C, xs, seq, 9);
        const int len1 = 3 + (int)(n % 3);
        const long it0 = (long)((n / 3) % 3);
        Model M(C, xs, mode);
        {
            StepPlanner pl(true, C, xs);
            pl.s1_must_wait = true;  // (the entry launches are on the first stream)
            run_stretch(M, pl, it0, seq, len1);
        }
        M.idle();
        {
            StepPlanner pl(true, C, xs);  // armed: nothing of this call is on the first stream yet
            run_stretch(M, pl, it0 + len1, seq + len1, 4);
        }
        tally(t, M, seq, len1 + 4);
    }
}

}  // namespace

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    const uint64_t seed = strtoull(argv[1], nullptr, 10);
    const int shapes[3][2] = {{8, 4}, {5, 2}, {MAXC, 10}};
    for (const auto &sh : shapes)
        for (int mode = 0; mode < 3; mode++) {
            if (mode == 0 || sh[0] <= 8) {  // (a mutation is seen at 5 and 8 chains over every sequence, at 20 over the random ones)
                Tally t;
                exhaustive(sh[0], sh[1], 4, mode, t);
                printf("Q %d %d x4 %d %ld %ld %s\n", sh[0], sh[1], mode, t.seqs, t.violations, t.violations ? t.first.c_str() : "-");
            }
            {
                Tally t;
                two_stretches(seed, sh[0], sh[1], mode, t);
                printf("Q %d %d two %d %ld %ld %s\n", sh[0], sh[1], mode, t.seqs, t.violations, t.violations ? t.first.c_str() : "-");
            }
        }
    return 0;
}
