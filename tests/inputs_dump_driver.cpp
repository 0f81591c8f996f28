// Dump driver of the input front end (C ABI of include/tamcmc_io.h only): for every `.model` file on the command line it calls the
// local loader for slices 0-8, the global and the red-giant loader, and prints ONE RECORD PER CALL -- the return code, then either the
// text of tamcmc_io_last_error() or every field of the inputs (doubles as %a).  With `--variants <scratch file>` it does the same for
// every variant of each file: the three families of parser_fuzz_driver.cpp (every prefix, every single-line deletion, the twelve
// junk substitutions), the prior keyword and the numbers of every common-parameter line replaced, and a list of hand-written edits
// that reach the builders' own refusals.  Two builds of csrc/host_io.cpp behave alike exactly when their outputs are equal.
//
// Record:  "== <file> | <variant> | <loader>[ <slice>]" / "rc <code>" / then on failure "error <text>", on success tab-separated lines
//   nparams, model_id, prior_class, model_name, range, dnu, c_l, plength, extra and per parameter
//   "p <i> <name> <prior name> <relax> <prior id> <value> <prior 0..3>".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <functional>
#include <sstream>
#include <string>
#include <vector>

#include "../include/tamcmc_io.h"

typedef std::vector<std::string> Lines;
static const double RESOL = 0.01;

static void record(const std::string &file, const std::string &variant, const char *loader, int rc, tamcmc_inputs *in) {
    std::printf("== %s | %s | %s\nrc %d\n", file.c_str(), variant.c_str(), loader, rc);
    if (rc != TAMCMC_IO_OK) {
        std::printf("error %s\n", tamcmc_io_last_error());
        return;
    }
    const int N = tamcmc_inputs_nparams(in);
    std::vector<double> params((size_t)N), priors((size_t)4 * N);
    std::vector<int32_t> relax((size_t)N), sw((size_t)N);
    int32_t plength[11], model_id = 0, prior_class = 0;
    double extra[10], range[2], dnu = 0, c_l = 0;
    tamcmc_inputs_get(in, params.data(), relax.data(), priors.data(), sw.data(), plength, extra, range, &model_id, &prior_class, &dnu, &c_l);
    std::printf("nparams\t%d\nmodel_id\t%d\nprior_class\t%d\nmodel_name\t%s\n", N, model_id, prior_class, tamcmc_inputs_model_name(in));
    std::printf("range\t%a\t%a\ndnu\t%a\nc_l\t%a\nplength", range[0], range[1], dnu, c_l);
    for (int k = 0; k < 11; k++) std::printf("\t%d", plength[k]);
    std::printf("\nextra");
    for (int k = 0; k < 10; k++) std::printf("\t%a", extra[k]);
    std::printf("\n");
    for (int i = 0; i < N; i++)
        std::printf("p\t%d\t%s\t%s\t%d\t%d\t%a\t%a\t%a\t%a\t%a\n", i, tamcmc_inputs_name(in, i), tamcmc_inputs_prior_name(in, i), relax[(size_t)i],
                    sw[(size_t)i], params[(size_t)i], priors[(size_t)i], priors[(size_t)N + i], priors[(size_t)2 * N + i], priors[(size_t)3 * N + i]);
    tamcmc_inputs_free(in);
}

static void all_loaders(const std::string &path, const std::string &file, const std::string &variant) {
    for (int slice = 0; slice <= 8; slice++) {
        tamcmc_inputs *in = nullptr;
        const int rc = tamcmc_io_load_model_local(path.c_str(), slice, RESOL, &in);
        record(file, variant, ("local " + std::to_string(slice)).c_str(), rc, in);
    }
    tamcmc_inputs *in = nullptr;
    int rc = tamcmc_io_load_model_global(path.c_str(), RESOL, &in);
    record(file, variant, "global", rc, in);
    in = nullptr;
    rc = tamcmc_io_load_model_asymptotic(path.c_str(), RESOL, &in);
    record(file, variant, "asymptotic", rc, in);
}

static Lines words(const std::string &s) {
    std::istringstream is(s);
    Lines w;
    for (std::string t; is >> t;) w.push_back(t);
    return w;
}
static std::string join(const Lines &w) {
    std::string s;
    for (const auto &t : w) s += (s.empty() ? "" : "  ") + t;
    return s;
}
static bool numeric(const std::string &w) {
    char *end = nullptr;
    std::strtod(w.c_str(), &end);
    return end != w.c_str() && *end == 0;
}
static bool is_mode(const Lines &w) { return !w.empty() && (w[0] == "p" || w[0] == "g" || w[0] == "co"); }
// a line of "# Controls and priors for common parameters": first word neither a number nor one of # ! * p g co
static bool is_common(const std::string &ln) {
    const Lines w = words(ln);
    return !w.empty() && !numeric(w[0]) && !is_mode(w) && w[0][0] != '#' && w[0][0] != '!' && w[0][0] != '*';
}
static bool is_eigen(const Lines &w) {
    if (w.size() != 6) return false;
    for (const auto &t : w)
        if (!numeric(t)) return false;
    return true;
}
// the "hyper priors" rows: the lines that start with a number between the last mode line and the first eigen-table row
static std::vector<size_t> hyper_rows(const Lines &L) {
    size_t last_mode = 0, first_eigen = L.size();
    for (size_t k = 0; k < L.size(); k++)
        if (is_mode(words(L[k]))) last_mode = k;
    for (size_t k = L.size(); k-- > last_mode;)
        if (is_eigen(words(L[k]))) first_eigen = k;
    std::vector<size_t> rows;
    for (size_t k = last_mode + 1; k < first_eigen; k++) {
        const Lines w = words(L[k]);
        if (!w.empty() && numeric(w[0])) rows.push_back(k);
    }
    return rows;
}
static long find_first_word(const Lines &L, const char *name) {
    for (size_t k = 0; k < L.size(); k++) {
        const Lines w = words(L[k]);
        if (!w.empty() && w[0] == name) return (long)k;
    }
    return -1;
}

struct Hand { const char *name; std::function<bool(Lines &)> edit; };  // edit returns false where the file has nothing to edit

static bool set_mode_flags(Lines &L, const char *flags) {
    for (auto &ln : L) {
        Lines w = words(ln);
        if (is_mode(w) && w.size() >= 3) ln = w[0] + " " + w[1] + " " + w[2] + " " + flags;
    }
    return true;
}
static bool replace_inclination(Lines &L, const Lines &by) {
    const long k = find_first_word(L, "Inclination");
    if (k < 0) return false;
    L.erase(L.begin() + k);
    L.insert(L.begin() + k, by.begin(), by.end());
    return true;
}
static bool keep_l0_eigen_rows(Lines &L, int keep) {
    Lines out;
    for (const auto &ln : L) {
        const Lines w = words(ln);
        if (is_eigen(w) && std::strtod(w[0].c_str(), nullptr) == 0 && keep-- <= 0) continue;
        out.push_back(ln);
    }
    L = out;
    return true;
}
static bool edit_hyper(Lines &L, size_t row, const std::function<void(Lines &)> &f) {
    const auto rows = hyper_rows(L);
    if (row >= rows.size()) return false;
    Lines w = words(L[rows[row]]);
    f(w);
    L[rows[row]] = join(w);
    return true;
}
static bool set_numax(Lines &L, const char *line) {
    for (auto &ln : L)
        if (ln.compare(0, 2, "!n") == 0) { ln = line; return true; }
    return false;
}

static const char *COS = "sqrt(splitting_a1).cosi  Uniform  0.5  0.0  1.2", *SIN = "sqrt(splitting_a1).sini  Uniform  0.4  0.0  1.2";
static const std::vector<Hand> hand_edits = {
    {"degree 4", [](Lines &L) {  // the last mode line becomes an l = 4 mode
         for (size_t k = L.size(); k-- > 0;) {
             Lines w = words(L[k]);
             if (is_mode(w) && w.size() >= 3) { w[1] = "4"; L[k] = join(w); return true; }
         }
         return false;
     }},
    {"range without modes", [](Lines &L) {
         for (auto &ln : L)
             if (!ln.empty() && ln[0] == '*') ln = "* 1.0 2.0";
         return true;
     }},
    {"no l=0 eigen row", [](Lines &L) { return keep_l0_eigen_rows(L, 0); }},
    {"one l=0 eigen row", [](Lines &L) { return keep_l0_eigen_rows(L, 1); }},
    {"mode flags 0 0 0", [](Lines &L) { return set_mode_flags(L, "0 0 0"); }},
    {"mode flags 1 0 1", [](Lines &L) { return set_mode_flags(L, "1 0 1"); }},
    {"mode flags absent", [](Lines &L) { return set_mode_flags(L, ""); }},
    {"lone cosi for Inclination", [](Lines &L) { return replace_inclination(L, {COS}); }},
    {"cosi and sini for Inclination", [](Lines &L) { return replace_inclination(L, {COS, SIN}); }},
    {"cosi and sini after Inclination", [](Lines &L) { L.push_back(COS); L.push_back(SIN); return true; }},
    {"no hyper rows", [](Lines &L) {
         const auto rows = hyper_rows(L);
         for (size_t k = rows.size(); k-- > 0;) L.erase(L.begin() + (long)rows[k]);
         return !rows.empty();
     }},
    {"hyper rows 0 and 1 swapped", [](Lines &L) {
         const auto rows = hyper_rows(L);
         if (rows.size() < 2) return false;
         std::swap(L[rows[0]], L[rows[1]]);
         return true;
     }},
    {"hyper row 0 one column", [](Lines &L) { return edit_hyper(L, 0, [](Lines &w) { w.resize(1); }); }},
    {"hyper row 1 one column", [](Lines &L) { return edit_hyper(L, 1, [](Lines &w) { w.resize(1); }); }},
    {"hyper row 1 a number short", [](Lines &L) { return edit_hyper(L, 1, [](Lines &w) { if (w.size() > 3) w.pop_back(); }); }},
    {"hyper row 0 Fix", [](Lines &L) { return edit_hyper(L, 0, [](Lines &w) { if (w.size() > 1) w[1] = "Fix"; }); }},
    {"hyper row 1 Uniform", [](Lines &L) { return edit_hyper(L, 1, [](Lines &w) { if (w.size() > 1) w[1] = "Uniform"; }); }},
    {"numax negative", [](Lines &L) { return set_numax(L, "!n -5.0 1.0"); }},
    {"numax zero", [](Lines &L) { return set_numax(L, "!n 0.0 1.0"); }},
    {"numax without uncertainty", [](Lines &L) { return set_numax(L, "!n 113.78"); }},
    {"numax with a negative uncertainty", [](Lines &L) { return set_numax(L, "!n 950.0 -1.0"); }},
    {"no model_type, no bias_type", [](Lines &L) {
         const long a = find_first_word(L, "model_type");
         if (a >= 0) L.erase(L.begin() + a);
         const long b = find_first_word(L, "bias_type");
         if (b >= 0) L.erase(L.begin() + b);
         return a >= 0 || b >= 0;
     }},
    {"bias_type 0", [](Lines &L) {
         const long b = find_first_word(L, "bias_type");
         if (b >= 0) L[(size_t)b] = "bias_type  Fix  0.";
         return b >= 0;
     }},
};

// lines appended to the common parameters, each alone and together with the switch to squared amplitudes: keywords the fixtures
// do not hold, their lower-case spellings, keywords of the other dialects (which a loader must leave unread), later lines
// overriding earlier ones
static const char *AMP = "fit_squareAmplitude_instead_Height  bool  1";
static const char *appended[] = {
    "fit_squareAmplitude_instead_Height  bool  0", "fit_squareAmplitude_instead_Height  Fix  1", "trunc_c  Uniform  20.", "trunc_c  Fix  20.",
    "trunc_c  Fix  -3.", "trunc_c  30.", "Frequency  Gaussian  1  2  3  4  5", "Frequency  GUG  0  0  0  0.5  0.6", "frequency  Uniform  0",
    "Height  Fix_Auto  2.0  3.0", "Amplitude  Fix_Auto  2.0  3.0", "amplitude  Jeffreys  2.0  3.0  5000.", "height  Uniform  1.0  2.0  3000.",
    "width  Jeffreys  0.05  0.1  8.0", "Width  Fix_Auto  1", "Width  Uniform  0.05  0.1  8.0", "splitting_a1  Gaussian  0.6  0.6  0.1",
    "Splitting_a1  Fix  0.9", "splitting_a3  Uniform  0.01  -0.1  0.1", "asphericity_eta  Uniform  1e-5  0.0  1e-3", "Asphericity_eta  Fix_Auto  0",
    "Asphericity_eta  Fix_Auto  1", "asymetry  Uniform  10.  -50.  50.", "inclination  Uniform  90.0  0.0  90.0", "Inclination  Fix  30.0",
    "visibility_l1  Uniform  1.4  0.0  3.0", "visibility_l2  Fix  0.6", "visibility_l3  Uniform  0.07  0.0  0.5", "freq_smoothness  bool  0  3.5",
    "Freq_smoothness  Fix  0  3.5", "delta01  Uniform  0.01  -0.1  0.1", "sigma_Hl1  Uniform  0.1  0.0  1.0", "a1_env  Fix  0.1", "Rot_core  Fix  0.7",
    "eta0_switch  Fix  1", "eta0_switch  Uniform  1", "model_type  Fix  1.", "bias_type  Fix  2.", "a1_0  Fix  0.5", "a7_0  Fix  0.5",
    "model_fullname  model_MS_Global_aj_HarveyLike", "model_fullname  model_MS_local_Hnlm"};

int main(int argc, char **argv) {
    int first = 1;
    std::string scratch;
    if (argc > 2 && std::strcmp(argv[1], "--variants") == 0) { scratch = argv[2]; first = 3; }
    if (argc <= first) {
        std::fprintf(stderr, "usage: %s [--variants <scratch file>] file.model ...\n", argv[0]);
        return 2;
    }
    long variants = 0;
    for (int a = first; a < argc; a++) {
        const std::string path = argv[a], file = path.substr(path.find_last_of('/') + 1);
        all_loaders(path, file, "base");
        if (scratch.empty()) continue;
        std::ifstream f(path.c_str());
        Lines lines;
        for (std::string ln; std::getline(f, ln);) lines.push_back(ln);
        auto run = [&](const Lines &ls, const std::string &variant) {
            {
                std::ofstream o(scratch.c_str());
                for (const auto &l : ls) o << l << "\n";
            }
            all_loaders(scratch, file, variant);
            variants++;
        };
        for (size_t cut = 0; cut <= lines.size(); cut++) run(Lines(lines.begin(), lines.begin() + (long)cut), "prefix " + std::to_string(cut));
        for (size_t del = 0; del < lines.size(); del++) {
            Lines ls(lines);
            ls.erase(ls.begin() + (long)del);
            run(ls, "delete " + std::to_string(del));
        }
        for (size_t k = 0; k < lines.size(); k++) {
            int j = 0;
            for (const char *junk : {"", "#", "!", "* 1", "p", "p 9 x y z", "1 2", "name", "name prior", "a=b", "!G:", "1e999 nan -inf"}) {
                Lines ls(lines);
                ls[k] = junk;
                run(ls, "junk " + std::to_string(k) + " " + std::to_string(j++));
            }
        }
        for (size_t k = 0; k < lines.size(); k++) {
            if (!is_common(lines[k])) continue;
            const Lines w = words(lines[k]);
            for (const char *kw : {"Fix", "Fix_Auto", "bool", "Uniform", "GUG", "Gaussian", "Nonsense", "7.5"}) {
                Lines ls(lines), v(w);
                if (v.size() < 2) v.push_back(kw);
                else v[1] = kw;
                ls[k] = join(v);
                run(ls, "keyword " + std::to_string(k) + " " + kw);
            }
            Lines ls(lines), v(w.begin(), w.begin() + (w.size() < 2 ? 1 : 2));
            ls[k] = join(v);
            run(ls, "numbers dropped " + std::to_string(k));
            v.push_back("95");
            ls[k] = join(v);
            run(ls, "numbers 95 " + std::to_string(k));
        }
        for (size_t k = 0; k < lines.size(); k++) {  // the first number of a numeric line becomes -2
            Lines w = words(lines[k]);
            if (w.empty() || !numeric(w[0])) continue;
            w[0] = "-2";
            Lines ls(lines);
            ls[k] = join(w);
            run(ls, "first number -2 " + std::to_string(k));
        }
        for (const auto &h : hand_edits) {
            Lines ls(lines);
            if (h.edit(ls)) run(ls, std::string("hand: ") + h.name);
        }
        for (const char *extra : appended) {
            Lines ls(lines);
            ls.push_back(extra);
            run(ls, std::string("appended: ") + extra);
            ls.push_back(AMP);
            run(ls, std::string("appended with amplitudes: ") + extra);
        }
        Lines ls(lines);
        ls.push_back(AMP);
        run(ls, "appended: amplitudes");
    }
    if (!scratch.empty()) std::fprintf(stderr, "variants %ld\n", variants);
    return 0;
}
