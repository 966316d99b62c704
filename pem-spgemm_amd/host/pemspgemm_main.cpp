// pemspgemm -- command-line front end with the reference's surface (spgemm.cu:720-1568):
//     pemspgemm <matrix.mtx> [0|1] [any third argument => C = A*A^T]
// reads one Matrix-Market file, forms C = A*A (or A*A^T), times WARMUP + REPEAT passes of
// step1+step2+step3, prints the reference's report, appends the reference's 14 CSV columns
// to ./pemspgemm_benchmark_result.csv and, when the 2nd argument is non-zero, writes the
// sorted COO result to /tmp/SPGEMM_RESULT_{NNZ,ROWS,COLS,VALS}.txt.
// Host C++ over the C ABI of libpemspgemm_hip.so.  The only HIP calls in this file are those of DevBuf: the dense device
// vectors that --reduce, --trsv, --argreduce, --bfs, --bfs-parents, --spmm and --sddmm hand to the library.
// Layout: Options (parse_args, validate), the helpers every stage shares, --gpus, then one function per stage; main() at the
// end of the file is the table of contents.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cctype>
#include <cerrno>
#include <cmath>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <numeric>
#include <thread>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <sys/stat.h>
#include <vector>
#include "../../include/pem_host.h"
#include "../../include/pem_mgpu.h"
#include "../../include/pem_spgemm.h"
#include <hip/hip_runtime_api.h>

static int env_int(const char *name, int dflt)
{
    const char *s = getenv(name);
    return s && *s ? atoi(s) : dflt;
}

#define CHECK(expr)                                                              \
    do {                                                                         \
        pem_status _s = (expr);                                                  \
        if (_s != PEM_OK) {                                                      \
            fprintf(stderr, "pemspgemm: %s failed (%d): %s\n", #expr, _s, pem_last_error()); \
            return 2;                                                            \
        }                                                                        \
    } while (0)

using Clock = std::chrono::high_resolution_clock;
static double ms_since(Clock::time_point t0) { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); }

// ------------------------------------------------------------------------------------------------------------------
// Options: every flag beyond the reference's grammar, the positional arguments that remain, and what validate() derives.
// ------------------------------------------------------------------------------------------------------------------
static const char *const semiring_names[] = {"plus_times", "min_plus", "max_plus", "max_times", "plus_pair", "lor_land"};   // pem_semiring
static const int add_ops[] = {PEM_BINOP_PLUS, PEM_BINOP_MIN, PEM_BINOP_MAX, PEM_BINOP_MAX, PEM_BINOP_PLUS, PEM_BINOP_LOR};   // by pem_semiring
static const char *const binop_names[] = {"plus", "times", "min", "max", "lor", "land"};                                    // by pem_binop
static const char *const dup_names[] = {"plus", "times", "min", "max", "lor", "land", "first", "second"};   // pem_binop, PEM_DUP_FIRST, PEM_DUP_SECOND
static const char *const select_names[] = {"tril",     "triu",     "diag",     "offdiag",  "row_le",   "row_gt",   "col_le", "col_gt",
                                           "value_eq", "value_ne", "value_lt", "value_le", "value_gt", "value_ge", "abs_gt"};   // pem_select_op
static const char *const apply_names[] = {"identity", "abs", "ainv", "minv", "sqrt", "one", "plus",
                                          "times",    "min", "max",  "div",  "rdiv", "rminus", "powi"};   // pem_apply_op
static const char *const topk_names[] = {"largest", "smallest", "abs_largest"};   // pem_topk_order
static const char *const dim_names[] = {"rows", "cols"};                           // pem_reduce_dim
static const char *const scale_flags[2] = {"--row-scale", "--col-scale"};
static const char *const extract_flags[2] = {"--extract-rows", "--extract-cols"};
static const char *const assign_flags[2] = {"--assign-rows", "--assign-cols"};
static const char *const stack_flags[2] = {"--hstack", "--vstack"};

struct Options {
    // Beyond the reference: `--B <file.mtx>` multiplies by a second matrix instead of A itself,
    // `--out <file.mtx>` writes C as a Matrix-Market file.  They are stripped before the reference's own grammar.
    const char *b_path = nullptr, *out_path = nullptr;
    const char *cache_dir = nullptr;   // --cache <dir>: see make_tiling
    // `--fp32` computes in float: the values are rounded once at conversion, step 3 runs one fmaf per product.
    bool fp32 = false;
    // `--standin NAME [--scale S]`: the seeded C++ stand-in generator takes the place of the file (no SuiteSparse
    // file exists offline); NAME then stands where the path stood, and the remaining positional arguments keep their meaning.
    const char *standin = nullptr;
    double standin_scale = 1.0;
    int ngpu = 0;             // --gpus N (0: the reference's single-device path): see run_gpus
    bool tune_split = true;   // --no-tune-split
    int nchunks = -1;         // --chunks K: chunks per rank of the overlapped pass (-1: from C's size, 0: off)
    // `--mask <M.mtx>` computes the masked product C<M> = A*B: only the entries at M's stored positions (pem_cplan_create_masked);
    // with `--mask-complement` only those where M stores nothing.  M has C's shape; the flop count stays the unmasked product's.
    const char *mask_path = nullptr;
    bool mask_complement = false;
    // `--semiring NAME`: step 3 reduces under plus_times (default), min_plus, max_plus, max_times,
    // plus_pair or lor_land; C's structure, the flop count (the tile product's) and the CSV columns do not change.
    const char *semiring_name = nullptr;
    int power = 0;                                                  // --power K (0: off): see power_prologue
    const char *add_path = nullptr;                                 // --add D.mtx [--alpha x] [--beta y]: see add_stage
    double add_alpha = 1.0, add_beta = 1.0;
    const char *apply_spec = nullptr;                               // --apply OP[:THUNK]: see apply_stage
    const char *scale_paths[2] = {nullptr, nullptr};                // --row-scale r.mtx, --col-scale c.mtx [--scale-op OP]: see scale_stage
    const char *scale_op_name = nullptr;
    const char *select_spec = nullptr;                              // --select OP[:THUNK]: see select_stage
    const char *topk_spec = nullptr;                                // --topk DIM:ORDER:K: see topk_stage
    const char *extract_paths[2] = {nullptr, nullptr};              // --extract-rows I.mtx, --extract-cols J.mtx: see extract_stage
    const char *assign_into = nullptr, *assign_accum_name = nullptr;   // --assign-into D.mtx, --assign-accum OP: see assign_stage
    const char *assign_paths[2] = {nullptr, nullptr};               // --assign-rows I.mtx, --assign-cols J.mtx
    const char *kron_path = nullptr, *kron_op_name = nullptr;       // --kron K.mtx [--kron-op OP]: see kron_stage
    const char *stack_paths[2] = {nullptr, nullptr};                // --hstack F.mtx, --vstack F.mtx: see stack_stage
    const char *dup_name = nullptr;                                 // --dup OP: see tiling_from_coo
    const char *reduce_spec = nullptr;                              // --reduce rows|cols[:OP]: see reduce_stage
    const char *bfs_spec = nullptr;                                 // --bfs SRC: see bfs_stage
    const char *argreduce_spec = nullptr;                           // --argreduce rows|cols:min|max: see argreduce_stage
    const char *bfs_parents_spec = nullptr;                         // --bfs-parents SRC: see bfs_parents_stage
    const char *spmm_path = nullptr;                                // --spmm X.mtx: see spmm_stage
    const char *sddmm_path = nullptr, *sddmm_y_path = nullptr;      // --sddmm X.mtx [--sddmm-y Y.mtx]: see sddmm_stage
    const char *sampled_path = nullptr;                             // --sampled S.mtx [--sampled-bt]: see sampled_stage
    bool sampled_bt = false, triangles = false;                     // --triangles: see sampled_stage
    const char *trsv_spec = nullptr, *rhs_path = nullptr;           // --trsv lower|upper[:unit] [--rhs b.mtx]: see trsv_stage
    bool ilu0 = false;                                              // --ilu0: see ilu0_stage
    const char *solve_spec = nullptr, *precond_name = nullptr;      // --solve cg|bicgstab [--precond none|jacobi|ilu0]: see solve_stage
    const char *rtol_spec = nullptr, *max_iters_spec = nullptr;     // --rtol R, --max-iters N
    const char *amg_kind = nullptr;                                 // --amg smoothed|plain: --solve's multigrid preconditioner
    const char *colour_spec = nullptr;                              // --colour SEED: see colour_stage
    bool colour_natural = false;                                    // --colour-natural: equal priorities
    bool components = false;                                        // --components: see components_stage
    const char *aggregate_spec = nullptr;                           // --aggregate SEED: see aggregate_stage

    // what is left for the reference's grammar: args[0] the program, args[1] the input, then [0|1] and the A*A^T argument
    std::string standin_path;
    std::vector<char *> args;
    const char *input() const { return args[1]; }

    // derived by validate()
    int WARMUP = 1, REPEAT = 10;
    bool fastest = false, save = false, aat = false;
    int semiring = PEM_SEMIRING_PLUS_TIMES;
    int apply_op = -1;
    double apply_thunk = 0.0;
    int scale_op = PEM_BINOP_TIMES;
    std::vector<double> scale_vec[2];
    int select_op = -1;
    double select_thunk = 0.0;
    int topk_dim = -1, topk_order = -1;
    long long topk_k = 0;
    std::vector<int32_t> extract_idx[2], assign_idx[2];   // 0-based
    int assign_accum = PEM_ACCUM_NONE;
    int kron_op = PEM_BINOP_TIMES;
    int dup = -1;                                         // -1: no --dup, duplicates are refused
    int64_t spmm_rows = 0, spmm_k = 0, sddmm_xrows = 0, sddmm_yrows = 0, sddmm_k = 0;
    std::vector<double> spmm_x, sddmm_x, sddmm_y;         // row-major
    int reduce_dim = -1, reduce_op = -1;
    long long bfs_src = 0;                                // 1-based
    int argreduce_dim = -1, argreduce_op = -1;
    long long bfs_parents_src = 0;                        // 1-based
    int trsv_uplo = -1;                                   // PEM_TRSV_LOWER / PEM_TRSV_UPPER
    bool trsv_unit = false;
    std::vector<double> rhs;                              // --rhs' values
    int solve_method = -1;                                // PEM_KRYLOV_CG / PEM_KRYLOV_BICGSTAB
    int solve_precond = 0;                                // 0 none, 1 jacobi, 2 ilu0
    double solve_rtol = 1e-8;
    long long solve_max_iters = 1000;
    int amg_smooth = -1;                                  // --amg: 1 smoothed, 0 plain
    uint32_t colour_seed = 0;
    uint32_t aggregate_seed = 0;
    const char *colour_flag() const { return colour_spec ? "--colour" : colour_natural ? "--colour-natural" : nullptr; }
};

// Strips the flags above out of argv; what is not one of them (or is one without its value) stays positional.
static void parse_args(int argc, char *argv[], Options *o)
{
    const char *scale = nullptr, *gpus = nullptr, *power = nullptr, *alpha = nullptr, *beta = nullptr, *chunks = nullptr;
    const struct {
        const char *name, **value;
    } valued[] = {{"--B", &o->b_path}, {"--standin", &o->standin}, {"--scale", &scale}, {"--gpus", &gpus}, {"--out", &o->out_path},
                  {"--cache", &o->cache_dir}, {"--mask", &o->mask_path}, {"--semiring", &o->semiring_name}, {"--power", &power},
                  {"--add", &o->add_path}, {"--alpha", &alpha}, {"--beta", &beta}, {"--select", &o->select_spec},
                  {"--extract-rows", &o->extract_paths[0]}, {"--extract-cols", &o->extract_paths[1]}, {"--assign-into", &o->assign_into},
                  {"--assign-rows", &o->assign_paths[0]}, {"--assign-cols", &o->assign_paths[1]}, {"--assign-accum", &o->assign_accum_name},
                  {"--reduce", &o->reduce_spec}, {"--bfs", &o->bfs_spec}, {"--spmm", &o->spmm_path}, {"--sddmm", &o->sddmm_path},
                  {"--sddmm-y", &o->sddmm_y_path}, {"--chunks", &chunks}, {"--apply", &o->apply_spec},
                  {"--row-scale", &o->scale_paths[0]}, {"--col-scale", &o->scale_paths[1]}, {"--scale-op", &o->scale_op_name},
                  {"--kron", &o->kron_path}, {"--kron-op", &o->kron_op_name}, {"--topk", &o->topk_spec},
                  {"--dup", &o->dup_name}, {"--hstack", &o->stack_paths[0]}, {"--vstack", &o->stack_paths[1]},
                  {"--argreduce", &o->argreduce_spec}, {"--bfs-parents", &o->bfs_parents_spec}, {"--sampled", &o->sampled_path},
                  {"--trsv", &o->trsv_spec}, {"--rhs", &o->rhs_path}, {"--colour", &o->colour_spec},
                  {"--aggregate", &o->aggregate_spec}, {"--solve", &o->solve_spec}, {"--precond", &o->precond_name},
                  {"--rtol", &o->rtol_spec}, {"--max-iters", &o->max_iters_spec}, {"--amg", &o->amg_kind}};
    const struct {
        const char *name;
        bool *flag, value;
    } plain[] = {{"--fp32", &o->fp32, true}, {"--mask-complement", &o->mask_complement, true}, {"--no-tune-split", &o->tune_split, false},
                 {"--sampled-bt", &o->sampled_bt, true}, {"--triangles", &o->triangles, true}, {"--ilu0", &o->ilu0, true},
                 {"--colour-natural", &o->colour_natural, true}, {"--components", &o->components, true}};
    o->args.assign(1, argv[0]);
    for (int r = 1; r < argc; ++r) {
        bool taken = false;
        for (const auto &v : valued)
            if (!taken && !strcmp(argv[r], v.name) && r + 1 < argc) *v.value = argv[++r], taken = true;
        for (const auto &p : plain)
            if (!taken && !strcmp(argv[r], p.name)) *p.flag = p.value, taken = true;
        if (!taken) o->args.push_back(argv[r]);
    }
    if (scale) o->standin_scale = atof(scale);
    if (gpus) o->ngpu = atoi(gpus);
    if (power) o->power = atoi(power);
    if (alpha) o->add_alpha = atof(alpha);
    if (beta) o->add_beta = atof(beta);
    if (chunks) o->nchunks = atoi(chunks);
    if (o->standin) {
        o->standin_path = std::string("standin:") + o->standin;
        o->args.insert(o->args.begin() + 1, const_cast<char *>(o->standin_path.c_str()));
    }
}

// The clash rules: a flag and what it refuses, the first one present being the one named.
static const struct ClashRule {
    const char *flag, *refused[12], *why;
} clash_rules[] = {
    {"--power", {"--gpus", "--mask", "--B", "the A*A^T argument"}, " (A^K multiplies A by itself on one device)"},
    {"--add", {"--gpus", "--mask", "--power"}, ""},
    {"--select", {"--gpus", "--power"}, ""},
    {"--extract-rows", {"--gpus", "--power"}, ""},
    {"--extract-cols", {"--gpus", "--power"}, ""},
    {"--assign-into", {"--gpus", "--power"}, ""},
    {"--spmm", {"--gpus", "--power", "--reduce"}, ""},
    {"--sddmm", {"--gpus", "--power", "--reduce", "--spmm"}, ""},
    {"--reduce", {"--gpus", "--power"}, ""},
    {"--bfs", {"--gpus", "--power", "--reduce", "--spmm", "--sddmm"}, ""},
    {"--argreduce", {"--gpus", "--power", "--reduce", "--bfs", "--spmm", "--sddmm"}, ""},
    {"--bfs-parents", {"--gpus", "--power", "--reduce", "--bfs", "--argreduce", "--spmm", "--sddmm"}, ""},
    {"--trsv", {"--gpus", "--power", "--reduce", "--bfs", "--argreduce", "--spmm", "--sddmm"}, ""},
    {"--solve", {"--gpus", "--power", "--trsv", "--reduce", "--bfs", "--argreduce", "--bfs-parents", "--spmm", "--sddmm"}, ""},
    {"--colour", {"--gpus", "--power", "--reduce", "--bfs", "--argreduce", "--bfs-parents", "--trsv", "--spmm", "--sddmm"}, ""},
    {"--colour-natural", {"--gpus", "--power", "--reduce", "--bfs", "--argreduce", "--bfs-parents", "--trsv", "--spmm", "--sddmm"}, ""},
    {"--components",
     {"--gpus", "--power", "--reduce", "--bfs", "--argreduce", "--bfs-parents", "--trsv", "--spmm", "--sddmm", "--colour", "--colour-natural"},
     ""},
    {"--aggregate",
     {"--gpus", "--power", "--reduce", "--bfs", "--argreduce", "--bfs-parents", "--trsv", "--spmm", "--sddmm", "--colour", "--colour-natural",
      "--components"},
     ""},
    {"--gpus", {"--mask"}, " (masked products run on one device)"},
    {"--apply", {"--gpus", "--power"}, ""},
    {"--row-scale", {"--gpus", "--power"}, ""},
    {"--col-scale", {"--gpus", "--power"}, ""},
    {"--kron", {"--gpus"}, ""},
    {"--topk", {"--gpus", "--power"}, ""},
    {"--hstack", {"--gpus", "--vstack"}, ""},
    {"--vstack", {"--gpus"}, ""},
    {"--ilu0", {"--gpus", "--power"}, ""},
    {"--dup", {"--gpus", "--cache"}, ""},   // (a cached tiling would depend on the op, which its key does not carry)
};

// Prints the refusal and returns true when `flag` (which is present) meets something its rule refuses.
static bool clashes(const Options &o, const char *flag)
{
    const struct {
        const char *name;
        bool present;
    } given[] = {{"--gpus", o.ngpu > 0},       {"--mask", o.mask_path != nullptr}, {"--power", o.power != 0},
                 {"--B", o.b_path != nullptr}, {"the A*A^T argument", o.aat},      {"--reduce", o.reduce_spec != nullptr},
                 {"--spmm", o.spmm_path != nullptr}, {"--sddmm", o.sddmm_path != nullptr},
                 {"--cache", o.cache_dir != nullptr}, {"--vstack", o.stack_paths[1] != nullptr},
                 {"--bfs", o.bfs_spec != nullptr}, {"--argreduce", o.argreduce_spec != nullptr},
                 {"--bfs-parents", o.bfs_parents_spec != nullptr}, {"--trsv", o.trsv_spec != nullptr},
                 {"--colour", o.colour_spec != nullptr}, {"--colour-natural", o.colour_natural},
                 {"--components", o.components}};
    for (const ClashRule &rule : clash_rules) {
        if (strcmp(rule.flag, flag)) continue;
        for (const char *other : rule.refused)
            for (const auto &g : given)
                if (other && !strcmp(other, g.name) && g.present) {
                    printf("%s does not combine with %s%s. Exiting.\n", flag, other, rule.why);
                    return true;
                }
    }
    return false;
}

// the position of `s` among n names, or -1
static int find_name(const char *const *names, int n, const std::string &s)
{
    for (int i = 0; i < n; ++i)
        if (s == names[i]) return i;
    return -1;
}

// Opens a Matrix-Market `array ... general` file and reads its header up to the size line (rows x cols); `integer_too` admits
// the integer field next to real.  Returns "" with *f open at the first value, else what is wrong (*f is closed by the caller
// whenever it is not null).
static std::string open_mm_array(const char *path, bool integer_too, FILE **f, long long *m, long long *n)
{
    *f = fopen(path, "r");
    if (!*f) return "cannot open the file";
    char line[4096];
    if (!fgets(line, sizeof line, *f)) return "empty file";
    char banner[64] = "", object[64] = "", format[64] = "", field[64] = "", symmetry[64] = "";
    if (sscanf(line, "%63s %63s %63s %63s %63s", banner, object, format, field, symmetry) != 5) return "no Matrix-Market header";
    for (char *t : {banner, object, format, field, symmetry})
        for (; *t; ++t) *t = (char)tolower((unsigned char)*t);
    if (strcmp(banner, "%%matrixmarket") || strcmp(object, "matrix")) return "no Matrix-Market header";
    if (strcmp(format, "array")) return std::string("a ") + format + " file, not an array (dense) file";
    if (strcmp(field, "real") && !(integer_too && !strcmp(field, "integer")))
        return std::string("a ") + field + (integer_too ? " file, not an integer or real one" : " file, not a real one");
    if (strcmp(symmetry, "general")) return std::string("a ") + symmetry + " array, not a general one";
    do {
        if (!fgets(line, sizeof line, *f)) return "no size line";
    } while (line[0] == '%');
    if (sscanf(line, "%lld %lld", m, n) != 2 || *m < 0 || *n < 0) return "bad size line";
    return "";
}

// X of --spmm / --sddmm, Y of --sddmm-y: a Matrix-Market `array real general` file (values column by column), returned row-major
// (x[j * k + c]).  Returns 0, or 1 after the refusal.  (pem_mm_read reads coordinate files only.)
static int read_dense_array(const char *flag, const char *path, int64_t *rows, int64_t *k, std::vector<double> *x)
{
    FILE *f = nullptr;
    long long m = -1, n = -1;
    std::string err = open_mm_array(path, false, &f, &m, &n);
    if (err.empty()) x->assign((size_t)m * (size_t)n, 0.0);
    for (long long c = 0; c < n && err.empty(); ++c)
        for (long long j = 0; j < m && err.empty(); ++j)
            if (fscanf(f, "%lf", &(*x)[(size_t)j * (size_t)n + (size_t)c]) != 1) err = "fewer values than rows x cols";
    if (f) fclose(f);
    *rows = m, *k = n;
    if (!err.empty()) printf("%s %s: %s (want a Matrix-Market array real general file). Exiting.\n", flag, path, err.c_str());
    return err.empty() ? 0 : 1;
}

// An index list of --extract-rows / --extract-cols / --assign-rows / --assign-cols: a Matrix-Market `array` file of one column,
// `integer` or `real` with integral values, holding 1-based indices like a coordinate file; idx receives them 0-based.  Returns 0,
// or 1 after the refusal.
static int read_index_array(const char *flag, const char *path, std::vector<int32_t> *idx)
{
    FILE *f = nullptr;
    long long m = -1, n = -1;
    std::string err = open_mm_array(path, true, &f, &m, &n);
    if (err.empty() && n != 1) err = "an array of " + std::to_string(n) + " columns, not of one";
    if (err.empty() && (m < 1 || m > 2147483647ll)) err = "a list of " + std::to_string(m) + " indices, not of 1 .. 2^31 - 1";
    if (err.empty()) idx->assign((size_t)m, 0);
    for (long long j = 0; j < m && err.empty(); ++j) {
        double v;
        if (fscanf(f, "%lf", &v) != 1)
            err = "fewer values than the size line says";
        else if (!(std::floor(v) == v))
            err = "index " + std::to_string(j + 1) + " is not an integer";
        else if (!(v >= 1.0 && v <= 2147483647.0))
            err = "index " + std::to_string(j + 1) + " is out of range (indices are 1-based)";
        else
            (*idx)[(size_t)j] = (int32_t)((long long)v - 1);
    }
    if (f) fclose(f);
    if (!err.empty()) printf("%s %s: %s (want a Matrix-Market array file of one column of 1-based indices). Exiting.\n", flag, path, err.c_str());
    return err.empty() ? 0 : 1;
}

// --semiring, --power, --add / --alpha / --beta
static int validate_product(Options *o)
{
    if (o->mask_complement && !o->mask_path) {
        printf("--mask-complement needs --mask <M.mtx>. Exiting.\n");
        return 1;
    }
    if (o->semiring_name && (o->semiring = find_name(semiring_names, 6, o->semiring_name)) < 0) {
        printf("--semiring %s: unknown semiring (plus_times, min_plus, max_plus, max_times, plus_pair, lor_land). Exiting.\n", o->semiring_name);
        return 1;
    }
    if (o->ngpu > 0 && o->semiring != PEM_SEMIRING_PLUS_TIMES) {
        printf("--gpus does not combine with --semiring %s (the multi-GPU path multiplies under plus_times). Exiting.\n", semiring_names[o->semiring]);
        return 1;
    }
    if (o->power != 0 && o->power < 2) {
        printf("--power %d: K must be at least 2. Exiting.\n", o->power);
        return 1;
    }
    if (o->power != 0 && clashes(*o, "--power")) return 1;
    const bool scaled = o->add_alpha != 1.0 || o->add_beta != 1.0;
    if (o->add_path) {
        if (clashes(*o, "--add")) return 1;
        if (scaled && o->semiring != PEM_SEMIRING_PLUS_TIMES) {
            printf("--add: --alpha / --beta other than 1 need the plus_times semiring, not %s. Exiting.\n", semiring_names[o->semiring]);
            return 1;
        }
    } else if (scaled) {
        printf("--alpha / --beta need --add <D.mtx>. Exiting.\n");
        return 1;
    }
    return 0;
}

// --select: the op by name (pem_select_op) and its thunk
static int validate_select(Options *o)
{
    if (!o->select_spec) return 0;
    if (clashes(*o, "--select")) return 1;
    const char *colon = strchr(o->select_spec, ':');
    const std::string name = colon ? std::string(o->select_spec, (size_t)(colon - o->select_spec)) : std::string(o->select_spec);
    o->select_op = find_name(select_names, 15, name);
    if (o->select_op < 0) {
        printf("--select %s: unknown op %s (tril, triu, diag, offdiag, row_le, row_gt, col_le, col_gt, value_eq, value_ne, value_lt, "
               "value_le, value_gt, value_ge, abs_gt). Exiting.\n", o->select_spec, name.c_str());
        return 1;
    }
    if (colon) {
        char *end = nullptr;
        o->select_thunk = strtod(colon + 1, &end);
        if (end == colon + 1 || *end != '\0') {
            printf("--select %s: the thunk %s does not parse as a number. Exiting.\n", o->select_spec, colon + 1);
            return 1;
        }
    }
    if (o->select_op <= PEM_SELECT_COL_GT && !(std::floor(o->select_thunk) == o->select_thunk && std::fabs(o->select_thunk) <= 2147483648.0)) {
        printf("--select %s: the positional op %s needs an integral thunk k with |k| <= 2^31. Exiting.\n", o->select_spec, name.c_str());
        return 1;
    }
    return 0;
}

// --extract-rows / --extract-cols and --assign-into: the accum by name and the lists read up front, so that a bad option or
// file is refused before any work
static int validate_lists(Options *o)
{
    for (int q = 0; q < 2; ++q) {
        if (!o->extract_paths[q]) continue;
        if (clashes(*o, extract_flags[q])) return 1;
        if (read_index_array(extract_flags[q], o->extract_paths[q], &o->extract_idx[q])) return 1;
    }
    if (!o->assign_into) {
        const char *lone = o->assign_paths[0] ? assign_flags[0] : o->assign_paths[1] ? assign_flags[1] : o->assign_accum_name ? "--assign-accum" : nullptr;
        if (lone) printf("%s needs --assign-into <D.mtx>. Exiting.\n", lone);
        return lone ? 1 : 0;
    }
    if (clashes(*o, "--assign-into")) return 1;
    if (o->assign_accum_name && (o->assign_accum = find_name(binop_names, 6, o->assign_accum_name)) == PEM_ACCUM_NONE) {
        printf("--assign-accum %s: unknown op (plus, times, min, max, lor, land). Exiting.\n", o->assign_accum_name);
        return 1;
    }
    for (int q = 0; q < 2; ++q) {
        if (!o->assign_paths[q]) continue;
        if (read_index_array(assign_flags[q], o->assign_paths[q], &o->assign_idx[q])) return 1;
        std::vector<int32_t> sorted(o->assign_idx[q]);
        std::sort(sorted.begin(), sorted.end());
        const auto dup = std::adjacent_find(sorted.begin(), sorted.end());
        if (dup != sorted.end()) {
            printf("%s %s: index %d is repeated; assign is defined for lists without repeats only. Exiting.\n", assign_flags[q], o->assign_paths[q],
                   *dup + 1);
            return 1;
        }
    }
    return 0;
}

// --spmm and --sddmm: X and Y read up front, so that a bad file is refused before any work
static int validate_dense(Options *o)
{
    if (o->spmm_path) {
        if (clashes(*o, "--spmm")) return 1;
        if (read_dense_array("--spmm", o->spmm_path, &o->spmm_rows, &o->spmm_k, &o->spmm_x)) return 1;
    }
    if (o->sddmm_y_path && !o->sddmm_path) {
        printf("--sddmm-y needs --sddmm <X.mtx>. Exiting.\n");
        return 1;
    }
    if (!o->sddmm_path) return 0;
    if (clashes(*o, "--sddmm")) return 1;
    if (read_dense_array("--sddmm", o->sddmm_path, &o->sddmm_xrows, &o->sddmm_k, &o->sddmm_x)) return 1;
    o->sddmm_yrows = o->sddmm_xrows;
    if (o->sddmm_y_path) {
        int64_t ky = 0;
        if (read_dense_array("--sddmm-y", o->sddmm_y_path, &o->sddmm_yrows, &ky, &o->sddmm_y)) return 1;
        if (ky != o->sddmm_k) {
            printf("--sddmm-y %s: Y has %lld columns, X has %lld. Exiting.\n", o->sddmm_y_path, (long long)ky, (long long)o->sddmm_k);
            return 1;
        }
    }
    return 0;
}

// --reduce: the dimension and the op (pem_binop; default: the semiring's additive op); --bfs: the 1-based source; --argreduce:
// the dimension and min or max; --bfs-parents: the 1-based source; --trsv: the triangle and :unit, --rhs read up front; --ilu0: what it does not combine with;
// --colour: the seed, --colour-natural: nothing to read; either refuses every other vector output; --components: those and the two
static int validate_vectors(Options *o)
{
    if (o->components && clashes(*o, "--components")) return 1;
    if (o->colour_spec && o->colour_natural) {
        printf("--colour does not combine with --colour-natural (a seed hashes the priorities, --colour-natural makes them equal). Exiting.\n");
        return 1;
    }
    if (o->colour_flag() && clashes(*o, o->colour_flag())) return 1;
    if (o->colour_spec) {
        char *end = nullptr;
        const unsigned long long seed = strtoull(o->colour_spec, &end, 10);
        if (end == o->colour_spec || *end != '\0' || o->colour_spec[0] == '-' || seed > 0xFFFFFFFFull) {
            printf("--colour %s: want a seed in 0 .. 4294967295. Exiting.\n", o->colour_spec);
            return 1;
        }
        o->colour_seed = (uint32_t)seed;
    }
    if (o->aggregate_spec) {
        if (clashes(*o, "--aggregate")) return 1;
        char *end = nullptr;
        const unsigned long long seed = strtoull(o->aggregate_spec, &end, 10);
        if (end == o->aggregate_spec || *end != '\0' || o->aggregate_spec[0] == '-' || seed > 0xFFFFFFFFull) {
            printf("--aggregate %s: want a seed in 0 .. 4294967295. Exiting.\n", o->aggregate_spec);
            return 1;
        }
        o->aggregate_seed = (uint32_t)seed;
    }
    if (o->ilu0 && clashes(*o, "--ilu0")) return 1;
    if (o->rhs_path && !o->trsv_spec && !o->solve_spec) {
        printf("--rhs needs --trsv lower|upper[:unit]. Exiting.\n");
        return 1;
    }
    if (!o->solve_spec && (o->precond_name || o->rtol_spec || o->max_iters_spec)) {
        printf("--precond / --rtol / --max-iters need --solve cg|bicgstab. Exiting.\n");
        return 1;
    }
    if (o->amg_kind) {
        if (!o->solve_spec) {
            printf("--amg needs --solve cg|bicgstab. Exiting.\n");
            return 1;
        }
        if (o->precond_name) {
            printf("--amg does not combine with --precond. Exiting.\n");
            return 1;
        }
        o->amg_smooth = !strcmp(o->amg_kind, "smoothed") ? 1 : !strcmp(o->amg_kind, "plain") ? 0 : -1;
        if (o->amg_smooth < 0) {
            printf("--amg %s: unknown kind (smoothed, plain). Exiting.\n", o->amg_kind);
            return 1;
        }
    }
    if (o->solve_spec) {
        if (clashes(*o, "--solve")) return 1;
        for (const char *other : {o->colour_flag(), o->components ? "--components" : nullptr, o->aggregate_spec ? "--aggregate" : nullptr})
            if (other) {
                printf("--solve does not combine with %s. Exiting.\n", other);
                return 1;
            }
        o->solve_method = !strcmp(o->solve_spec, "cg") ? PEM_KRYLOV_CG : !strcmp(o->solve_spec, "bicgstab") ? PEM_KRYLOV_BICGSTAB : -1;
        if (o->solve_method < 0) {
            printf("--solve %s: unknown method (cg, bicgstab). Exiting.\n", o->solve_spec);
            return 1;
        }
        if (o->precond_name) {
            static const char *const names[] = {"none", "jacobi", "ilu0"};
            o->solve_precond = -1;
            for (int k = 0; k < 3; ++k)
                if (!strcmp(o->precond_name, names[k])) o->solve_precond = k;
            if (o->solve_precond < 0) {
                printf("--precond %s: unknown preconditioner (none, jacobi, ilu0). Exiting.\n", o->precond_name);
                return 1;
            }
        }
        if (o->rtol_spec) {
            char *end = nullptr;
            o->solve_rtol = strtod(o->rtol_spec, &end);
            if (end == o->rtol_spec || *end != '\0' || !(o->solve_rtol >= 0.0)) {
                printf("--rtol %s: want a number >= 0. Exiting.\n", o->rtol_spec);
                return 1;
            }
        }
        if (o->max_iters_spec) {
            char *end = nullptr;
            o->solve_max_iters = strtoll(o->max_iters_spec, &end, 10);
            if (end == o->max_iters_spec || *end != '\0' || o->solve_max_iters < 0) {
                printf("--max-iters %s: want an integer >= 0. Exiting.\n", o->max_iters_spec);
                return 1;
            }
        }
        if (!o->rhs_path) {
            printf("--solve %s needs --rhs b.mtx. Exiting.\n", o->solve_spec);
            return 1;
        }
        int64_t n = 0, k = 0;
        if (read_dense_array("--rhs", o->rhs_path, &n, &k, &o->rhs)) return 1;
        if (k != 1) {
            printf("--rhs %s: an array of %lld columns, not of one. Exiting.\n", o->rhs_path, (long long)k);
            return 1;
        }
    }
    if (o->trsv_spec) {
        if (clashes(*o, "--trsv")) return 1;
        if (o->bfs_parents_spec) {
            printf("--trsv does not combine with --bfs-parents. Exiting.\n");
            return 1;
        }
        const char *colon = strchr(o->trsv_spec, ':');
        const std::string tri = colon ? std::string(o->trsv_spec, (size_t)(colon - o->trsv_spec)) : std::string(o->trsv_spec);
        o->trsv_uplo = tri == "lower" ? PEM_TRSV_LOWER : tri == "upper" ? PEM_TRSV_UPPER : -1;
        if (o->trsv_uplo < 0) {
            printf("--trsv %s: unknown triangle %s (lower, upper). Exiting.\n", o->trsv_spec, tri.c_str());
            return 1;
        }
        if (colon && strcmp(colon + 1, "unit")) {
            printf("--trsv %s: want lower|upper[:unit]. Exiting.\n", o->trsv_spec);
            return 1;
        }
        o->trsv_unit = colon != nullptr;
        if (o->rhs_path) {
            int64_t n = 0, k = 0;
            if (read_dense_array("--rhs", o->rhs_path, &n, &k, &o->rhs)) return 1;
            if (k != 1) {
                printf("--rhs %s: an array of %lld columns, not of one. Exiting.\n", o->rhs_path, (long long)k);
                return 1;
            }
        }
    }
    o->reduce_op = add_ops[o->semiring];
    if (o->reduce_spec) {
        if (clashes(*o, "--reduce")) return 1;
        const char *colon = strchr(o->reduce_spec, ':');
        const std::string dim = colon ? std::string(o->reduce_spec, (size_t)(colon - o->reduce_spec)) : std::string(o->reduce_spec);
        o->reduce_dim = dim == "rows" ? PEM_REDUCE_ROWS : dim == "cols" ? PEM_REDUCE_COLS : -1;
        if (o->reduce_dim < 0) {
            printf("--reduce %s: unknown dimension %s (rows, cols). Exiting.\n", o->reduce_spec, dim.c_str());
            return 1;
        }
        if (colon && (o->reduce_op = find_name(binop_names, 6, colon + 1)) < 0) {
            printf("--reduce %s: unknown op %s (plus, times, min, max, lor, land). Exiting.\n", o->reduce_spec, colon + 1);
            return 1;
        }
    }
    if (o->bfs_spec) {
        if (clashes(*o, "--bfs")) return 1;
        char *end = nullptr;
        o->bfs_src = strtoll(o->bfs_spec, &end, 10);
        if (end == o->bfs_spec || *end != '\0' || o->bfs_src < 1) {
            printf("--bfs %s: want a 1-based vertex number. Exiting.\n", o->bfs_spec);
            return 1;
        }
    }
    if (o->argreduce_spec) {
        if (clashes(*o, "--argreduce")) return 1;
        const char *colon = strchr(o->argreduce_spec, ':');
        const std::string dim = colon ? std::string(o->argreduce_spec, (size_t)(colon - o->argreduce_spec)) : std::string(o->argreduce_spec);
        o->argreduce_dim = dim == "rows" ? PEM_REDUCE_ROWS : dim == "cols" ? PEM_REDUCE_COLS : -1;
        if (o->argreduce_dim < 0) {
            printf("--argreduce %s: unknown dimension %s (rows, cols). Exiting.\n", o->argreduce_spec, dim.c_str());
            return 1;
        }
        const std::string op = colon ? colon + 1 : "";
        o->argreduce_op = op == "min" ? PEM_BINOP_MIN : op == "max" ? PEM_BINOP_MAX : -1;
        if (o->argreduce_op < 0) {
            printf("--argreduce %s: want rows|cols:min|max; unknown op %s (min, max). Exiting.\n", o->argreduce_spec, op.c_str());
            return 1;
        }
    }
    if (o->bfs_parents_spec) {
        if (clashes(*o, "--bfs-parents")) return 1;
        char *end = nullptr;
        o->bfs_parents_src = strtoll(o->bfs_parents_spec, &end, 10);
        if (end == o->bfs_parents_spec || *end != '\0' || o->bfs_parents_src < 1) {
            printf("--bfs-parents %s: want a 1-based vertex number. Exiting.\n", o->bfs_parents_spec);
            return 1;
        }
    }
    return 0;
}

// --apply: the op by name (pem_apply_op) and its thunk; --row-scale / --col-scale / --scale-op: the op by name (pem_binop) and the
// vectors read up front, so that a bad option or file is refused before any work
static int validate_apply(Options *o)
{
    if (o->apply_spec) {
        if (clashes(*o, "--apply")) return 1;
        const char *colon = strchr(o->apply_spec, ':');
        const std::string name = colon ? std::string(o->apply_spec, (size_t)(colon - o->apply_spec)) : std::string(o->apply_spec);
        o->apply_op = find_name(apply_names, 14, name);
        if (o->apply_op < 0) {
            printf("--apply %s: unknown op %s (identity, abs, ainv, minv, sqrt, one, plus, times, min, max, div, rdiv, rminus, powi). Exiting.\n",
                   o->apply_spec, name.c_str());
            return 1;
        }
        if (colon) {
            char *end = nullptr;
            o->apply_thunk = strtod(colon + 1, &end);
            if (end == colon + 1 || *end != '\0') {
                printf("--apply %s: the thunk %s does not parse as a number. Exiting.\n", o->apply_spec, colon + 1);
                return 1;
            }
        }
        if (o->apply_op == PEM_APPLY_POWI && !(std::floor(o->apply_thunk) == o->apply_thunk && o->apply_thunk >= 1.0 && o->apply_thunk <= 64.0)) {
            printf("--apply %s: powi needs an integral thunk k in 1 .. 64. Exiting.\n", o->apply_spec);
            return 1;
        }
    }
    if (o->scale_op_name && !o->scale_paths[0] && !o->scale_paths[1]) {
        printf("--scale-op needs --row-scale <r.mtx> or --col-scale <c.mtx>. Exiting.\n");
        return 1;
    }
    for (int q = 0; q < 2; ++q)
        if (o->scale_paths[q] && clashes(*o, scale_flags[q])) return 1;
    if (o->scale_op_name && (o->scale_op = find_name(binop_names, 6, o->scale_op_name)) < 0) {
        printf("--scale-op %s: unknown op (plus, times, min, max, lor, land). Exiting.\n", o->scale_op_name);
        return 1;
    }
    for (int q = 0; q < 2; ++q) {
        if (!o->scale_paths[q]) continue;
        int64_t n = 0, k = 0;
        if (read_dense_array(scale_flags[q], o->scale_paths[q], &n, &k, &o->scale_vec[q])) return 1;
        if (k != 1) {
            printf("%s %s: an array of %lld columns, not of one. Exiting.\n", scale_flags[q], o->scale_paths[q], (long long)k);
            return 1;
        }
    }
    return 0;
}

// --kron / --kron-op: the op by name (pem_binop); K itself is read with the operands
static int validate_kron(Options *o)
{
    if (!o->kron_path) {
        if (o->kron_op_name) printf("--kron-op needs --kron <K.mtx>. Exiting.\n");
        return o->kron_op_name ? 1 : 0;
    }
    if (clashes(*o, "--kron")) return 1;
    if (o->kron_op_name && (o->kron_op = find_name(binop_names, 6, o->kron_op_name)) < 0) {
        printf("--kron-op %s: unknown op (plus, times, min, max, lor, land). Exiting.\n", o->kron_op_name);
        return 1;
    }
    return 0;
}

// --hstack / --vstack: one of the two, on one device; the file itself is read with the operands
static int validate_stack(Options *o)
{
    for (int k = 0; k < 2; ++k)
        if (o->stack_paths[k] && clashes(*o, stack_flags[k])) return 1;
    return 0;
}

// --topk DIM:ORDER:K: the dimension (pem_reduce_dim) and the order (pem_topk_order) by name, K an integer >= 0
static int validate_topk(Options *o)
{
    if (!o->topk_spec) return 0;
    if (clashes(*o, "--topk")) return 1;
    const std::string spec = o->topk_spec;
    const size_t c1 = spec.find(':'), c2 = c1 == std::string::npos ? c1 : spec.find(':', c1 + 1);
    const std::string dim = spec.substr(0, c1), order = c1 == std::string::npos ? std::string() : spec.substr(c1 + 1, c2 - c1 - 1),
                      kstr = c2 == std::string::npos ? std::string() : spec.substr(c2 + 1);
    if ((o->topk_dim = find_name(dim_names, 2, dim)) < 0) {
        printf("--topk %s: unknown dimension %s (rows, cols); the form is DIM:ORDER:K. Exiting.\n", o->topk_spec, dim.c_str());
        return 1;
    }
    if ((o->topk_order = find_name(topk_names, 3, order)) < 0) {
        printf("--topk %s: unknown order %s (largest, smallest, abs_largest); the form is DIM:ORDER:K. Exiting.\n", o->topk_spec, order.c_str());
        return 1;
    }
    char *end = nullptr;
    errno = 0;
    o->topk_k = strtoll(kstr.c_str(), &end, 10);
    if (kstr.empty() || !isdigit((unsigned char)kstr[0]) || *end != '\0' || errno != 0) {
        printf("--topk %s: K must be an integer >= 0, not %s. Exiting.\n", o->topk_spec, kstr.c_str());
        return 1;
    }
    return 0;
}

// --dup OP: the op by name (a pem_binop, first or second) under which every Matrix-Market operand's duplicates are folded
static int validate_dup(Options *o)
{
    if (!o->dup_name) return 0;
    if ((o->dup = find_name(dup_names, 8, o->dup_name)) < 0) {
        printf("--dup %s: unknown op (plus, times, min, max, lor, land, first, second). Exiting.\n", o->dup_name);
        return 1;
    }
    return clashes(*o, "--dup") ? 1 : 0;
}

// --sampled S.mtx [--sampled-bt], --triangles: each takes the place of the plan product, so whatever shapes that product or works
// on its result is refused by name
static int validate_sampled(Options *o)
{
    if (o->sampled_bt && !o->sampled_path) {
        printf("--sampled-bt needs --sampled <S.mtx>. Exiting.\n");
        return 1;
    }
    const char *const flag = o->sampled_path ? "--sampled" : o->triangles ? "--triangles" : nullptr;
    if (!flag) return 0;
    if (o->sampled_path && o->triangles) {
        printf("--triangles does not combine with --sampled (it is a sampled product of its own: L o (L*L^T) under plus_pair). Exiting.\n");
        return 1;
    }
    if (o->sampled_bt && o->aat) {
        printf("--sampled-bt does not combine with the A*A^T argument (both ask for B^T: --sampled-bt reads B's rows, the argument converts B^T). Exiting.\n");
        return 1;
    }
    const struct {
        const char *name;
        bool present;
    } plan_only[] = {{"--gpus", o->ngpu > 0}, {"--mask", o->mask_path != nullptr}, {"--power", o->power != 0}, {"--add", o->add_path != nullptr},
                     {"--apply", o->apply_spec != nullptr}, {"--row-scale", o->scale_paths[0] != nullptr}, {"--col-scale", o->scale_paths[1] != nullptr},
                     {"--select", o->select_spec != nullptr}, {"--topk", o->topk_spec != nullptr}, {"--extract-rows", o->extract_paths[0] != nullptr},
                     {"--extract-cols", o->extract_paths[1] != nullptr}, {"--assign-into", o->assign_into != nullptr}, {"--kron", o->kron_path != nullptr},
                     {"--hstack", o->stack_paths[0] != nullptr}, {"--vstack", o->stack_paths[1] != nullptr}, {"--reduce", o->reduce_spec != nullptr},
                     {"--bfs", o->bfs_spec != nullptr}, {"--argreduce", o->argreduce_spec != nullptr}, {"--bfs-parents", o->bfs_parents_spec != nullptr},
                     {"--spmm", o->spmm_path != nullptr}, {"--sddmm", o->sddmm_path != nullptr}, {"--cache", o->cache_dir != nullptr},
                     {"--trsv", o->trsv_spec != nullptr}, {"--ilu0", o->ilu0}, {"--colour", o->colour_spec != nullptr},
                     {"--colour-natural", o->colour_natural}, {"--components", o->components},
                     {"--aggregate", o->aggregate_spec != nullptr}, {"--solve", o->solve_spec != nullptr},
                     {"the 2nd argument 1 (the sorted COO files; use --out)", o->save}};
    for (const auto &f : plan_only)
        if (f.present) {
            printf("%s does not combine with %s (it takes the place of the plan product, and no stage runs after it). Exiting.\n", flag, f.name);
            return 1;
        }
    if (o->triangles) {
        const struct {
            const char *name;
            bool present;
        } own[] = {{"--B", o->b_path != nullptr}, {"the A*A^T argument", o->aat}, {"--semiring", o->semiring_name != nullptr}, {"--out", o->out_path != nullptr}};
        for (const auto &f : own)
            if (f.present) {
                printf("--triangles does not combine with %s (it counts the triangles of A's pattern and prints the count). Exiting.\n", f.name);
                return 1;
            }
    }
    return 0;
}

// Checks the options against each other and reads the files that can be refused before any work (index lists, X, Y).  Returns 0
// to go on, else the exit code after the refusal; the order of the checks decides which refusal a command with two faults gets.
static int validate(Options *o)
{
    if (o->args.size() <= 1 || o->args.size() > 4) {   // spgemm.cu:722-725
        printf("Provide a matrix market file path. Exiting.\n");
        return 1;
    }
    o->WARMUP = env_int("PEM_WARMUP", 1);                               // spgemm.cu:712-714
    o->REPEAT = env_int("PEM_REPEAT", 10);                              // reference Makefile:34 (-DREPEAT=10)
    o->fastest = env_int("PEM_FASTEST", 0) != 0;                        // spgemm.cu:1359-1363
    o->save = o->args.size() >= 3 && atoi(o->args[2]) != 0;             // spgemm.cu:1485 (the reference dereferences argv[2] unconditionally)
    o->aat = o->args.size() == 4;                                       // spgemm.cu:788: presence of a 3rd argument, value ignored
    for (auto step : {validate_product, validate_select, validate_lists, validate_dense, validate_vectors, validate_apply, validate_kron, validate_topk, validate_dup, validate_stack, validate_sampled})
        if (int rc = step(o)) return rc;
    if (o->ngpu > 0 && clashes(*o, "--gpus")) return 1;
    if (o->ngpu > 0 && (o->fp32 || o->cache_dir)) {
        printf("--gpus does not combine with --fp32 / --cache. Exiting.\n");
        return 1;
    }
    return 0;
}

// ------------------------------------------------------------------------------------------------------------------
// Helpers shared by the stages: ownership, input, tilings from COO, exports, device vectors, the writers.
// ------------------------------------------------------------------------------------------------------------------
struct CtxDeleter {   // tilings and plans are destroyed on the context that made them
    pem_ctx *ctx = nullptr;
    void operator()(pem_tiled *t) const { pem_tiled_destroy(ctx, t); }
    void operator()(pem_cplan *p) const { pem_cplan_destroy(ctx, p); }
    void operator()(pem_ctx *c) const { pem_ctx_destroy(c); }
};
using Tiled = std::unique_ptr<pem_tiled, CtxDeleter>;
using Plan = std::unique_ptr<pem_cplan, CtxDeleter>;
using Ctx = std::unique_ptr<pem_ctx, CtxDeleter>;

// out(ctx, p) stands where the ABI wants a T **: p owns what the call made once the full expression ends (std::out_ptr's shape)
template <class T>
struct Out {
    std::unique_ptr<T, CtxDeleter> &dst;
    pem_ctx *ctx;
    T *raw = nullptr;
    operator T **() { return &raw; }
    ~Out() { if (raw) dst = std::unique_ptr<T, CtxDeleter>(raw, CtxDeleter{ctx}); }
};
template <class T>
static Out<T> out(pem_ctx *ctx, std::unique_ptr<T, CtxDeleter> &dst) { return Out<T>{dst, ctx}; }

struct Coo : pem_coo {   // a host COO matrix, freed with its scope
    Coo() { memset(static_cast<pem_coo *>(this), 0, sizeof(pem_coo)); }
    ~Coo() { pem_coo_free(this); }
    Coo(const Coo &) = delete;
    Coo &operator=(const Coo &) = delete;
};

// the input: a Matrix-Market file (spgemm.cu:43-110), or "standin:NAME" for the seeded generator (--standin)
static int read_input(const Options &o, const char *path, pem_coo *out)
{
    if (!strncmp(path, "standin:", 8)) {
        const int rc = pem_standin_generate(path + 8, o.standin_scale, out);
        if (rc != 0) fprintf(stderr, "pemspgemm: --standin %s (scale %g): no such stand-in (have: %s) or bad scale\n", path + 8, o.standin_scale, pem_standin_names());
        return rc;
    }
    const int rc = pem_mm_read(path, 0, out);
    if (rc != 0) fprintf(stderr, "pemspgemm: %s\n", pem_host_last_error());
    return rc;
}

// the file name of a path, without its directories
static std::string base_name(const std::string &path)
{
    const size_t slash = path.find_last_of('/');
    return slash == std::string::npos ? path : path.substr(slash + 1);
}

// CSV (spgemm.cu:1424-1450); matrix name = file stem (the reference's regex needs a '/' in the path)
static void append_csv_row(const Options &o, pem_csv_record rec, const char *extra)
{
    std::string stem = base_name(o.input());
    if (stem.size() > 4 && stem.compare(stem.size() - 4, 4, ".mtx") == 0) stem.resize(stem.size() - 4);
    rec.matrix = stem.c_str();
    const char *csv = getenv("PEM_CSV") ? getenv("PEM_CSV") : "./pemspgemm_benchmark_result.csv";
    if (pem_csv_append(csv, &rec, extra) != 0) fprintf(stderr, "pemspgemm: %s\n", pem_host_last_error());
}

// COO -> tiling; under fp32 the values are rounded to float first.  dup < 0: a repeated (row, col) is refused (pem_tiled_from_coo);
// else `--dup OP`: the repeats -- a symmetric file's expansion may add some -- are folded under it in file order (pem_tiled_build)
static pem_status tiling_from_coo(pem_ctx *ctx, const pem_coo &m, bool fp32, int transpose, int dup, Tiled *t)
{
    if (!fp32)
        return dup < 0 ? pem_tiled_from_coo(ctx, m.rows, m.cols, m.nnz, m.I, m.J, m.V, transpose, out(ctx, *t))
                       : pem_tiled_build(ctx, m.rows, m.cols, m.nnz, m.I, m.J, m.V, transpose, dup, 0, out(ctx, *t));
    std::vector<float> vf((size_t)m.nnz);
    for (int64_t e = 0; e < m.nnz; ++e) vf[(size_t)e] = (float)m.V[e];
    return dup < 0 ? pem_tiled_from_coo_f32(ctx, m.rows, m.cols, m.nnz, m.I, m.J, vf.data(), transpose, out(ctx, *t))
                   : pem_tiled_build_f32(ctx, m.rows, m.cols, m.nnz, m.I, m.J, vf.data(), transpose, dup, 0, out(ctx, *t));
}

// the same with the refusal: 0, or 2 after the message
static int convert_or_refuse(pem_ctx *ctx, const char *path, const pem_coo &m, bool fp32, int transpose, int dup, Tiled *t)
{
    if (tiling_from_coo(ctx, m, fp32, transpose, dup, t) == PEM_OK) return 0;
    fprintf(stderr, "pemspgemm: conversion of %s failed: %s\n", path, pem_last_error());
    return 2;
}

struct Csr {   // a host CSR matrix, values widened to double whatever the value type
    int32_t rows = 0, cols = 0;   // filled by the export of a tiling only
    std::vector<int32_t> rp, ci;
    std::vector<double> v;
    int64_t nnz() const { return (int64_t)ci.size(); }
};

// One of the export entry points (two index arrays a and b, already of the right size like v), its values widened to double
template <class T>
static pem_status export_f64(pem_ctx *ctx, const T *src, bool fp32, pem_status (*f64)(pem_ctx *, const T *, int64_t *, int32_t *, int32_t *, double *),
                             pem_status (*f32)(pem_ctx *, const T *, int64_t *, int32_t *, int32_t *, float *), int32_t *a, int32_t *b,
                             std::vector<double> *v)
{
    int64_t nnz = 0;
    if (!fp32) return f64(ctx, src, &nnz, a, b, v->data());
    std::vector<float> vf(v->size());
    const pem_status s = f32(ctx, src, &nnz, a, b, vf.data());
    std::copy(vf.begin(), vf.end(), v->begin());
    return s;
}

static pem_status export_csr(pem_ctx *ctx, const pem_tiled *t, bool fp32, Csr *c)
{
    pem_tiled_info ti;
    if (pem_status s = pem_tiled_get_info(t, &ti)) return s;
    c->rows = ti.rows, c->cols = ti.cols;
    c->rp.resize((size_t)ti.rows + 1), c->ci.resize((size_t)ti.nnz), c->v.resize((size_t)ti.nnz);
    return export_f64(ctx, t, fp32, pem_tiled_export_csr, pem_tiled_export_csr_f32, c->rp.data(), c->ci.data(), &c->v);
}

static pem_status export_csr(pem_ctx *ctx, const pem_cplan *plan, const pem_cplan_info &ci, bool fp32, Csr *c)
{
    c->rp.resize((size_t)(ci.row_end - ci.row_begin) + 1), c->ci.resize((size_t)ci.nnz_c), c->v.resize((size_t)ci.nnz_c);
    return export_f64(ctx, plan, fp32, pem_c_export_csr, pem_c_export_csr_f32, c->rp.data(), c->ci.data(), &c->v);
}

// sorted COO (spgemm.cu:1493-1543): c->rp receives the row of every entry
static pem_status export_coo(pem_ctx *ctx, const pem_cplan *plan, const pem_cplan_info &ci, bool fp32, Csr *c)
{
    c->rp.resize((size_t)ci.nnz_c), c->ci.resize((size_t)ci.nnz_c), c->v.resize((size_t)ci.nnz_c);
    return export_f64(ctx, plan, fp32, pem_c_export_coo, pem_c_export_coo_f32, c->rp.data(), c->ci.data(), &c->v);
}

// A dense device vector of n values of VT (float under fp32, else double; 8 spare bytes), freed with its scope.
struct DevBuf {
    void *p = nullptr;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { if (p) (void)hipFree(p); }
    bool alloc(size_t n, size_t value_bytes) { return hipMalloc(&p, value_bytes * n + 8) == hipSuccess; }
    // a fresh buffer of n values holding h (which has n values, or none when n counts padding only)
    bool upload(const std::vector<double> &h, size_t n, bool fp32)
    {
        if (!alloc(n, fp32 ? 4 : 8)) return false;
        if (h.empty()) return true;
        if (!fp32) return hipMemcpy(p, h.data(), 8 * h.size(), hipMemcpyHostToDevice) == hipSuccess;
        const std::vector<float> f(h.begin(), h.end());
        return hipMemcpy(p, f.data(), 4 * f.size(), hipMemcpyHostToDevice) == hipSuccess;
    }
    bool download(std::vector<double> *h, size_t n, bool fp32) const
    {
        h->resize(n);
        if (!n) return true;
        if (!fp32) return hipMemcpy(h->data(), p, 8 * n, hipMemcpyDeviceToHost) == hipSuccess;
        std::vector<float> f(n);
        if (hipMemcpy(f.data(), p, 4 * n, hipMemcpyDeviceToHost) != hipSuccess) return false;
        std::copy(f.begin(), f.end(), h->begin());
        return true;
    }
};

static double sum_of(const std::vector<double> &v) { return std::accumulate(v.begin(), v.end(), 0.0); }

// "12 rows" when a list was given, else "all rows"
static std::string count_or_all(const char *list_path, size_t n, const char *what)
{
    return list_path ? std::to_string(n) + " " + what : std::string("all ") + what;
}

// refuses a list whose index lies beyond the matrix it indexes (`owner`, of dims[0] x dims[1])
static bool lists_in_range(const char *const flags[2], const char *const paths[2], const std::vector<int32_t> idx[2], const int dims[2], const char *owner)
{
    for (int q = 0; q < 2; ++q)
        for (size_t j = 0; j < idx[q].size(); ++j)
            if (idx[q][j] >= dims[q]) {
                printf("%s %s: index %zu is %d; %s has %d %s. Exiting.\n", flags[q], paths[q], j + 1, idx[q][j] + 1, owner, dims[q], q ? "columns" : "rows");
                return false;
            }
    return true;
}

// The sorted COO result files.  0, or 2 after the message.
static int save_coo_files(int64_t nnz, const int32_t *rows, const int32_t *cols, const double *vals)
{
    const char *dir = getenv("PEM_RESULT_DIR") ? getenv("PEM_RESULT_DIR") : "/tmp";
    printf("Saving results to %s/SPGEMM_RESULT_*.txt\n", dir);
    if (pem_write_result_files(dir, nnz, rows, cols, vals) == 0) return 0;
    fprintf(stderr, "pemspgemm: %s\n", pem_host_last_error());
    return 2;
}

// the same from CSR arrays: sorted (row, col) order = CSR order (spgemm.cu:1516-1519)
static int save_result_files(const std::vector<int32_t> &rowptr, const std::vector<int32_t> &cols, const std::vector<double> &vals)
{
    std::vector<int32_t> rows(cols.size());
    for (size_t r = 0; r + 1 < rowptr.size(); ++r)
        for (int32_t e = rowptr[r]; e < rowptr[r + 1]; ++e) rows[(size_t)e] = (int32_t)r;
    return save_coo_files((int64_t)cols.size(), rows.data(), cols.data(), vals.data());
}

// --out of a matrix: `letter` ("C", "R") names it in the closing line.  0, or 2 after the message.
static int write_mtx(const char *path, int32_t rows, int32_t cols, const Csr &c, const std::string &comment, const char *letter)
{
    if (pem_write_mtx_csr(path, rows, cols, c.rp.data(), c.ci.data(), c.v.data(), comment.c_str()) != 0) {
        fprintf(stderr, "pemspgemm: %s\n", pem_host_last_error());
        return 2;
    }
    printf("%s written to %s\n", letter, path);
    return 0;
}

// --out of a vector or dense matrix: a Matrix-Market `array <field> general` file of rows x cols, values column by column out of
// the row-major `values` (leading dimension ld), 9 significant digits under fp32 and 17 otherwise.  `what` names the content in
// the closing line and, behind `the`, in the error.  0, or 2 after the message.
static int write_mm_array(const char *path, const char *field, const std::string &comment, int64_t rows, int64_t cols, const std::vector<double> &values,
                          int64_t ld, bool fp32, const char *the, const char *what)
{
    FILE *f = fopen(path, "w");
    bool ok = f != nullptr;
    if (ok) {
        ok = fprintf(f, "%%%%MatrixMarket matrix array %s general\n%% %s by pemspgemm (pem-spgemm_amd)\n%lld %lld\n", field, comment.c_str(), (long long)rows,
                     (long long)cols) > 0;
        for (int64_t c = 0; ok && c < cols; ++c)
            for (int64_t i = 0; ok && i < rows; ++i) ok = fprintf(f, fp32 ? "%.9g\n" : "%.17g\n", values[(size_t)(i * ld + c)]) > 0;
        ok = fclose(f) == 0 && ok;
    }
    if (!ok) {
        fprintf(stderr, "pemspgemm: --out %s: cannot write %s%s\n", path, the, what);
        return 2;
    }
    printf("%s written to %s\n", what, path);
    return 0;
}

// ------------------------------------------------------------------------------------------------------------------
// --gpus N (beyond the single-GPU reference): one host thread and one context per device, A split into N
// tile-row blocks balanced on tile-level products, B whole on every device, steps 1-3 with no communication, then the
// path's one exchange step: the CSR slices gathered to device 0 over RCCL (libpemmgpu.so).  A pass is timed from the
// moment all ranks start to the moment the last one finishes; the gather is timed on its own (t_gather).
// ------------------------------------------------------------------------------------------------------------------
namespace {
struct Barrier {
    std::mutex mu;
    std::condition_variable cv;
    int n, waiting = 0;
    unsigned long gen = 0;
    explicit Barrier(int n_) : n(n_) {}
    void wait()
    {
        std::unique_lock<std::mutex> lk(mu);
        const unsigned long g = gen;
        if (++waiting == n) {
            waiting = 0;
            ++gen;
            cv.notify_all();
        } else {
            cv.wait(lk, [&] { return gen != g; });
        }
    }
};

struct MultiResult {
    double step1 = 0, step2 = 0, step3 = 0, total = 0, cold = 0, gather_ms = 0, conv_ms = 0;
    double a_conv_kernel_ms = 0, b_conv_kernel_ms = 0;
    uint64_t flop = 0;
    int64_t ntiles_c = 0, npairs = 0, nnz_c = 0, rows = 0;
    int32_t cols_b = 0;
    std::vector<int32_t> rowptr, colidx;
    std::vector<double> vals;
    bool gathered = false;
    // the measured re-cut of the row split, and the chunked pass with the gather overlapped (libpemmgpu.so)
    int tune_rounds = 0;
    double tune_first_max = 0, tune_best_max = 0;
    std::vector<int32_t> bounds;
    int chunks = 0;
    double chunk_pass_ms = 0, chunk_tail_ms = 0;
};
}   // namespace

static int run_multi(int ngpu, const pem_coo &ca, const pem_coo *cb, bool aat, bool want_c, int WARMUP, int REPEAT, bool fastest,
                     std::chrono::high_resolution_clock::time_point conv_start, MultiResult &res, bool tune_split, int nchunks)
{
    std::vector<int> devs((size_t)ngpu);
    for (int g = 0; g < ngpu; ++g) devs[(size_t)g] = g;
    pem_mgpu *m = nullptr;
    if (pem_mgpu_create(ngpu, devs.data(), &m) != PEM_OK) {
        fprintf(stderr, "pemspgemm: --gpus %d: %s\n", ngpu, pem_last_error());
        return 2;
    }
    std::vector<pem_tiled *> A((size_t)ngpu, nullptr), B((size_t)ngpu, nullptr);
    std::vector<pem_cplan *> plan((size_t)ngpu, nullptr);
    std::vector<int32_t> bounds((size_t)ngpu + 1, 0);
    std::vector<std::vector<double>> s1((size_t)ngpu), s2((size_t)ngpu), s3((size_t)ngpu);
    std::vector<double> wall;
    std::atomic<int> failed{0};
    std::vector<std::string> errs((size_t)ngpu);
    Barrier bar(ngpu);
    std::vector<int32_t> cur((size_t)ngpu + 1, 0);          // the cut being timed (split tuning)
    std::vector<double> weights, tune_ms((size_t)ngpu, 0.0);
    int mt_all = 0;
    bool tune_done = false;
    const pem_coo &b_src = cb ? *cb : ca;
    auto worker = [&](int g) {
        pem_ctx *ctx = pem_mgpu_ctx(m, g);
        auto fail = [&](const char *what) {
            errs[(size_t)g] = std::string(what) + ": " + pem_last_error();
            failed = 1;
        };
        // every device tiles B whole (replicated) and A whole (its plan covers only its tile-row block)
        if (pem_tiled_from_coo(ctx, ca.rows, ca.cols, ca.nnz, ca.I, ca.J, ca.V, 0, &A[(size_t)g]) != PEM_OK) fail("conversion of A");
        if (!failed) {
            if (cb || aat) {
                if (pem_tiled_from_coo(ctx, b_src.rows, b_src.cols, b_src.nnz, b_src.I, b_src.J, b_src.V, aat ? 1 : 0, &B[(size_t)g]) != PEM_OK)
                    fail("conversion of B");
            } else {
                B[(size_t)g] = A[(size_t)g];
            }
        }
        bar.wait();
        if (g == 0 && !failed) {
            pem_tiled_info ia, ib;
            pem_tiled_get_info(A[0], &ia);
            pem_tiled_get_info(B[0], &ib);
            if (ia.cols != ib.rows) {
                errs[0] = "inner dimensions differ";
                failed = 1;
            } else if (pem_split_tile_rows(ctx, A[0], B[0], ngpu, bounds.data()) != PEM_OK || pem_flop_count(ctx, A[0], B[0], &res.flop) != PEM_OK) {
                fail("row split");
            } else {
                mt_all = ia.tile_rows;
                weights.resize((size_t)mt_all);
                if (tune_split && ngpu > 1 && pem_tile_row_weights(ctx, A[0], B[0], weights.data()) != PEM_OK) fail("tile-row weights");
                cur = bounds;
            }
            res.rows = ia.rows;
            res.cols_b = ib.cols;
            res.a_conv_kernel_ms = ia.conv_tile_kernel_ms;
            res.b_conv_kernel_ms = ib.conv_tile_kernel_ms;
            res.conv_ms = std::chrono::duration<double, std::milli>(std::chrono::high_resolution_clock::now() - conv_start).count();
        }
        bar.wait();
        // Measure-and-recut of the row split (setup, before anything is timed; the Python harness' multigpu.tune_row_bounds): every
        // rank times twenty repeat passes of its block as a replayed graph, rank 0 re-cuts the blocks from the times
        // (pem_mgpu_recut_bounds) so that ranks whose rows cost more per unit of weight get fewer of them; up to three rounds, and a
        // later cut is only kept if it beats the first by 3 % (pass times move by that much from run to run).
        if (tune_split && ngpu > 1) {
            for (int rnd = 0; rnd <= 3 && !failed; ++rnd) {
                pem_cplan *tp = nullptr;
                if (pem_cplan_create(ctx, A[(size_t)g], B[(size_t)g], cur[(size_t)g], cur[(size_t)g + 1], &tp) != PEM_OK) fail("plan (split tuning)");
                pem_set_graph_replay(ctx, 1);
                for (int k = 0; k < 3 && !failed; ++k)
                    if (pem_spgemm(ctx, tp) != PEM_OK) fail("pem_spgemm (split tuning)");
                bar.wait();
                const auto t0 = std::chrono::high_resolution_clock::now();
                for (int k = 0; k < 20 && !failed; ++k)
                    if (pem_spgemm(ctx, tp) != PEM_OK) fail("pem_spgemm (split tuning)");
                tune_ms[(size_t)g] = std::chrono::duration<double, std::milli>(std::chrono::high_resolution_clock::now() - t0).count() / 20.0;
                pem_set_graph_replay(ctx, 0);
                if (tp) pem_cplan_destroy(ctx, tp);
                bar.wait();
                if (g == 0 && !failed) {
                    const double mx = *std::max_element(tune_ms.begin(), tune_ms.end()), mn = *std::min_element(tune_ms.begin(), tune_ms.end());
                    double mean = 0;
                    for (double x : tune_ms) mean += x / (double)ngpu;
                    if (rnd == 0) {
                        res.tune_first_max = res.tune_best_max = mx;
                        bounds = cur;
                    } else if (mx < res.tune_best_max && mx < 0.97 * res.tune_first_max) {
                        res.tune_best_max = mx;
                        bounds = cur;
                    }
                    res.tune_rounds = rnd + 1;
                    tune_done = rnd == 3 || mx <= 1.04 * mean;
                    if (!tune_done) {
                        std::vector<int32_t> nxt((size_t)ngpu + 1);
                        if (pem_mgpu_recut_bounds(ngpu, mt_all, weights.data(), cur.data(), tune_ms.data(), (rnd == 0 ? 0.6 : 0.5) * mn, nxt.data()) != PEM_OK)
                            tune_done = true;
                        else
                            cur = nxt;
                    }
                }
                bar.wait();
                if (tune_done) break;
            }
        }
        if (!failed && pem_cplan_create(ctx, A[(size_t)g], B[(size_t)g], bounds[(size_t)g], bounds[(size_t)g + 1], &plan[(size_t)g]) != PEM_OK)
            fail("plan");
        for (int n = 0; n < WARMUP + REPEAT; ++n) {
            bar.wait();
            const auto t0 = std::chrono::high_resolution_clock::now();
            if (!failed && pem_spgemm(ctx, plan[(size_t)g]) != PEM_OK) fail("pem_spgemm");
            bar.wait();   // the pass ends when the last rank has finished
            const double ms = std::chrono::duration<double, std::milli>(std::chrono::high_resolution_clock::now() - t0).count();
            pem_timings t;
            memset(&t, 0, sizeof t);
            pem_get_timings(ctx, &t);
            if (g == 0 && n == 0) res.cold = ms;
            if (n >= WARMUP) {
                s1[(size_t)g].push_back(t.step1_ms);
                s2[(size_t)g].push_back(t.step2_ms);
                s3[(size_t)g].push_back(t.step3_ms);
                if (g == 0) wall.push_back(ms);
            }
        }
    };
    std::vector<std::thread> th;
    for (int g = 0; g < ngpu; ++g) th.emplace_back(worker, g);
    for (auto &t : th) t.join();
    int rc = 0;
    if (failed) {
        for (int g = 0; g < ngpu; ++g)
            if (!errs[(size_t)g].empty()) fprintf(stderr, "pemspgemm: rank %d: %s\n", g, errs[(size_t)g].c_str());
        if (!errs[0].empty() && errs[0] == "inner dimensions differ") printf("inner dimensions differ. Exiting.\n");
        rc = errs[0] == "inner dimensions differ" ? 1 : 2;
    } else {
        // the pass an iteration is judged by: the slowest rank's step spans, the barrier-to-barrier wall
        size_t fidx = 0;
        if (fastest && !wall.empty()) fidx = (size_t)(std::min_element(wall.begin(), wall.end()) - wall.begin());
        auto pick = [&](const std::vector<double> &v) {
            if (v.empty()) return 0.0;
            if (fastest) return v[fidx];
            double s = 0;
            for (double x : v) s += x;
            return s / (double)v.size();
        };
        for (int g = 0; g < ngpu; ++g) {
            res.step1 = std::max(res.step1, pick(s1[(size_t)g]));
            res.step2 = std::max(res.step2, pick(s2[(size_t)g]));
            res.step3 = std::max(res.step3, pick(s3[(size_t)g]));
            pem_cplan_info ci;
            pem_cplan_get_info(plan[(size_t)g], &ci);
            res.ntiles_c += ci.ntiles_c;
            res.npairs += ci.npairs;
        }
        res.total = pick(wall);
        // the exchange step: CSR slices -> device 0 over RCCL
        int64_t nrows = 0, nnz = 0;
        if (pem_mgpu_gather_csr(m, plan.data(), 0, &nrows, &nnz, nullptr, nullptr, nullptr, nullptr) != PEM_OK) {
            fprintf(stderr, "pemspgemm: gather: %s\n", pem_last_error());
            rc = 2;
        } else {
            res.nnz_c = nnz;
            const char *ge = getenv("PEM_GATHER");
            const bool do_gather = want_c || (ge ? atoi(ge) != 0 : nnz <= 400000000ll);
            if (do_gather) {
                res.rowptr.resize((size_t)nrows + 1);
                res.colidx.resize((size_t)nnz);
                res.vals.resize((size_t)nnz);
                if (pem_mgpu_gather_csr(m, plan.data(), 0, &nrows, &nnz, res.rowptr.data(), res.colidx.data(), res.vals.data(), &res.gather_ms) != PEM_OK) {
                    fprintf(stderr, "pemspgemm: gather: %s\n", pem_last_error());
                    rc = 2;
                } else {
                    res.gathered = true;
                }
            }
        }
    }
    res.bounds = bounds;
    // the same product as ONE call with the exchange overlapped: every rank's block in `nchunks` chunks, chunk c travelling to
    // device 0 while chunk c + 1 computes (pem_mgpu_spgemm_gather_chunked; the Python harness' ChunkedRowBlock)
    if (rc == 0 && nchunks != 0 && res.nnz_c > 0) {
        int K = nchunks;
        if (K < 0) {                                         // from the bytes one rank sends: ~48 MB of CSR per chunk, 2 .. 8
            const double per_rank = 12.0 * (double)res.nnz_c / (double)ngpu;
            K = (int)std::max(2.0, std::min(8.0, std::ceil(per_rank / (48.0 * 1048576.0))));
        }
        std::vector<int32_t> cb_((size_t)ngpu * (size_t)K + 1, 0);
        std::vector<pem_cplan *> cp((size_t)ngpu * (size_t)K, nullptr);
        bool ok = pem_split_tile_rows(pem_mgpu_ctx(m, 0), A[0], B[0], ngpu * K, cb_.data()) == PEM_OK;
        for (int s = 0; ok && s < ngpu * K; ++s)
            ok = pem_cplan_create(pem_mgpu_ctx(m, s / K), A[(size_t)(s / K)], B[(size_t)(s / K)], cb_[(size_t)s], cb_[(size_t)s + 1], &cp[(size_t)s]) == PEM_OK;
        int64_t nr = 0, nz = 0;
        double pass = 0, tail = 0, sp = 0, st = 0;
        if (ok) ok = pem_mgpu_spgemm_gather_chunked(m, cp.data(), K, 0, &nr, &nz, nullptr, nullptr, nullptr, &pass, &tail) == PEM_OK;   // sizes, warm plans
        for (int n = 0; ok && n < REPEAT; ++n) {
            ok = pem_mgpu_spgemm_gather_chunked(m, cp.data(), K, 0, &nr, &nz, nullptr, nullptr, nullptr, &pass, &tail) == PEM_OK;
            sp += pass / REPEAT;
            st += tail / REPEAT;
        }
        if (ok && nz != res.nnz_c) {
            fprintf(stderr, "pemspgemm: chunked pass: %lld entries, the row-block pass had %lld\n", (long long)nz, (long long)res.nnz_c);
            ok = false;
        }
        if (ok) {
            res.chunks = K;
            res.chunk_pass_ms = sp;
            res.chunk_tail_ms = st;
        } else {
            fprintf(stderr, "pemspgemm: chunked pass: %s\n", pem_last_error());
            rc = 2;
        }
        for (int s = 0; s < ngpu * K; ++s)
            if (cp[(size_t)s]) pem_cplan_destroy(pem_mgpu_ctx(m, s / K), cp[(size_t)s]);
    }
    for (int g = 0; g < ngpu; ++g) {
        pem_ctx *ctx = pem_mgpu_ctx(m, g);
        if (plan[(size_t)g]) pem_cplan_destroy(ctx, plan[(size_t)g]);
        if (B[(size_t)g] && B[(size_t)g] != A[(size_t)g]) pem_tiled_destroy(ctx, B[(size_t)g]);
        if (A[(size_t)g]) pem_tiled_destroy(ctx, A[(size_t)g]);
    }
    pem_mgpu_destroy(m);
    return rc;
}

// the report, the CSV row (28 columns), the result files and --out of a --gpus run
static int report_multi(const Options &o, const MultiResult &mr, const pem_coo &ca, int64_t b_nnz)
{
    const int ngpu = o.ngpu;
    int rc = 0;
    const double kernel = mr.step1 + mr.step2 + mr.step3, malloc_ms = mr.total - kernel;
    const double gflops = mr.total > 0 ? (double)mr.flop * 2.0 / (mr.total * 1e6) : 0.0;
    const double gflops_x = mr.total + mr.gather_ms > 0 ? (double)mr.flop * 2.0 / ((mr.total + mr.gather_ms) * 1e6) : 0.0;
    const double ratio = mr.nnz_c ? (double)mr.flop / (double)mr.nnz_c : 0.0;
    printf("\n%d GPUs, row blocks of A balanced on tile-level products, B replicated\nwarm up %d time\naverage over %d iterations\n\n", ngpu, o.WARMUP, o.REPEAT);
    printf("<---Program done--->\n");
    printf("total conversion overhead----------------%.2fms\n\n", mr.conv_ms);
    printf("step1 - High Level Multiplication took---%.2fms\n", mr.step1);
    printf("step2 - Allocating C took----------------%.2fms\n", mr.step2);
    printf("step3 - Accumulation took----------------%.2fms\n\n", mr.step3);
    printf("pemSpGEMM took %.2fms ----- GFlops: %.2f\nKernel time %.2fms\nmalloc time %.2fms\n", mr.total, gflops, kernel, malloc_ms);
    printf("first pass (allocations + size read-backs) %.2fms\n", mr.cold);
    if (mr.gathered) printf("gather of C to GPU 0 over RCCL took %.2fms ----- GFlops with it: %.2f\n", mr.gather_ms, gflops_x);
    if (mr.tune_rounds > 0)
        printf("row split re-cut from measured pass times: %d round(s), slowest rank %.3fms -> %.3fms\n", mr.tune_rounds, mr.tune_first_max,
               mr.tune_best_max);
    printf("tile-row blocks:");
    for (size_t g = 0; g + 1 < mr.bounds.size(); ++g) printf(" [%d,%d)", mr.bounds[g], mr.bounds[g + 1]);
    printf("\n");
    if (mr.chunks > 0)
        printf("%d chunks per rank, gather overlapped: compute %.2fms + transfers still in flight %.2fms ----- GFlops with the exchange: %.2f\n",
               mr.chunks, mr.chunk_pass_ms, mr.chunk_tail_ms,
               mr.chunk_pass_ms + mr.chunk_tail_ms > 0 ? (double)mr.flop * 2.0 / ((mr.chunk_pass_ms + mr.chunk_tail_ms) * 1e6) : 0.0);
    printf("Flop count: %llu\n\nC tiles: %lld\nC nnz: %lld\nCompression ratio %.2f\n", (unsigned long long)mr.flop, (long long)mr.ntiles_c,
           (long long)mr.nnz_c, ratio);
    const double b_alg = 12.0 * ((double)ca.nnz + (double)b_nnz + (double)mr.nnz_c) + 4.0 * 3.0 * ((double)ca.rows + 1);
    const double frac_kernel = kernel > 0 ? b_alg / (kernel * 1e-3) / (8.0e12 * ngpu) : 0.0;
    const double frac_total = mr.total > 0 ? b_alg / (mr.total * 1e-3) / (8.0e12 * ngpu) : 0.0;
    const pem_csv_record rec = {nullptr, mr.flop, mr.nnz_c, ratio, mr.a_conv_kernel_ms, mr.b_conv_kernel_ms, mr.conv_ms,
                                mr.step1, mr.step2, mr.step3, mr.total, kernel, malloc_ms, gflops};
    char extra[320];
    // columns 15..: gpus, B_alg, roofline fraction (kernel, total), C tiles, live pairs, first-pass ms, gather ms (sequential),
    // chunks per rank, chunked pass ms, transfers still in flight after it ms, split-tuning rounds, slowest rank before / after (ms)
    snprintf(extra, sizeof extra, "%d,%.0f,%.4f,%.4f,%lld,%lld,%.2f,%.2f,%d,%.2f,%.2f,%d,%.3f,%.3f", ngpu, b_alg, frac_kernel, frac_total,
             (long long)mr.ntiles_c, (long long)mr.npairs, mr.cold, mr.gather_ms, mr.chunks, mr.chunk_pass_ms, mr.chunk_tail_ms, mr.tune_rounds,
             mr.tune_first_max, mr.tune_best_max);
    append_csv_row(o, rec, extra);
    if (!o.save)
        printf("Not saving results. Exiting.\n");
    else
        rc = save_result_files(mr.rowptr, mr.colidx, mr.vals);
    if (o.out_path) {
        if (pem_write_mtx_csr(o.out_path, (int32_t)mr.rows, mr.cols_b, mr.rowptr.data(), mr.colidx.data(), mr.vals.data(),
                              "C = A*B by pemspgemm (pem-spgemm_amd), row blocks gathered over RCCL") != 0) {
            fprintf(stderr, "pemspgemm: %s\n", pem_host_last_error());
            rc = 2;
        } else {
            printf("C written to %s\n", o.out_path);
        }
    }
    return rc;
}

// `--gpus N`: N tile-row blocks of A on N devices, C gathered to device 0 over RCCL (see run_multi); the blocks are
// re-cut from measured pass times first (`--no-tune-split` keeps the product-balanced cut), and the product is also run as
// `--chunks K` chunks per rank with the gather overlapped (default: K from C's size; 0: off).
static int run_gpus(const Options &o)
{
    auto conv_start_m = Clock::now();
    Coo ca, cb;
    if (read_input(o, o.input(), &ca) != 0 || (o.b_path && read_input(o, o.b_path, &cb) != 0)) return 1;
    if (!o.b_path && !o.aat && ca.rows != ca.cols) {
        printf("input is rectangular. Only AAt is possible. Exiting.\n");   // spgemm.cu:782-786
        return 1;
    }
    printf("MATRIX A\nfilepath: %s\nRows: %d\nCols: %d\nNnz: %lld\n", o.input(), ca.rows, ca.cols, (long long)ca.nnz);
    MultiResult mr;
    int rc = run_multi(o.ngpu, ca, o.b_path ? &cb : nullptr, o.aat, o.save || o.out_path, o.WARMUP, o.REPEAT, o.fastest, conv_start_m, mr, o.tune_split,
                       o.nchunks);
    if (rc == 0) rc = report_multi(o, mr, ca, o.b_path ? cb.nnz : ca.nnz);
    printf("CLEANING UP RESOURCES\n\n");
    return rc;
}

// ------------------------------------------------------------------------------------------------------------------
// The single-device path: the operands, then one function per stage, each leaving what it made in Result.
// ------------------------------------------------------------------------------------------------------------------
struct Operands {
    Tiled Sp;   // --sampled's S
    Tiled A, B_own, Mt, Dt, Into, Kt, St;   // B_own: B when it is a tiling of its own; Mt the mask, Dt --add's D, Into --assign-into's D, Kt --kron's K, St --hstack's / --vstack's F
    pem_tiled *B = nullptr;
    pem_tiled_info ia, ib;
    double conv_ms = 0.0;
};

struct Result {
    Tiled L_own;              // --power: A^(K-1), the last product's left operand
    pem_tiled *L = nullptr;   // A otherwise
    Tiled sum, app, scl, sel, top, ext, asg, krn, stk, sd, ilu;   // what --add, --apply, --row/col-scale, --select, --topk, --extract-*, --assign-into, --kron, --hstack / --vstack, --sddmm and --ilu0 made
    Plan plan;
    pem_cplan_info ci;
    pem_tiled *last = nullptr;          // the final result so far when it is a tiling (null: it is the plan's C) ...
    const char *last_name = "C";        // ... and what the report lines call it
    std::vector<double> red, bfs_levels, spmm_y;   // --reduce's vector, --bfs' levels, --spmm's Y (row-major), on the host
    std::vector<double> arg_idx, bfs_parents;      // --argreduce's indices, --bfs-parents' parents: 1-based, 0 for none
    std::vector<double> colours;                   // --colour's colours, 1-based
    std::vector<double> labels;                    // --components' labels, 1-based
    std::vector<double> aggregates;                // --aggregate's aggregate ids, 1-based
    std::vector<double> trsv_x;                    // --trsv's solution
    std::vector<double> solve_x;                   // --solve's solution
    int64_t spmm_ny = 0;
    Csr sd_csr;               // --sddmm: the sampled product, which serves --out and the COO files
    int rc = 0;               // 2 once a result file could not be written (the run still finishes)
    void now_last(const Tiled &t, const char *name) { last = t.get(), last_name = name; }
};

// The final result as a tiling, for one stage: borrows Result::last when there is one, else owns a tiling made from the plan's C
// for its own lifetime.  Every stage makes and drops its own, inside whatever it times.
struct Operand {
    Tiled own;
    pem_tiled *t = nullptr;
    pem_tiled_info info;
    pem_status open(pem_ctx *ctx, const Result &r)
    {
        t = r.last;
        if (!t) {
            if (pem_status s = pem_tiled_from_cplan(ctx, r.plan.get(), 0, out(ctx, own))) return s;
            t = own.get();
        }
        return PEM_OK;
    }
};

// One tiling = (source file, transposed?).  `--cache <dir>` keeps each tiling as <dir>/<stem>.<A|AT>.pemtile and,
// while the .mtx is unchanged (size + mtime), loads it instead of parsing and converting; else the file is parsed + converted
// and then saved there.
struct Source {
    const char *path;
    Coo coo;
    bool read = false;
};
static int make_tiling(const Options &o, pem_ctx *ctx, Source &src, int transpose, Tiled *t, int *cache_hits, int *cache_misses)
{
    std::string cpath;
    pem_cache_key key;
    memset(&key, 0, sizeof key);
    bool keyed = false;
    struct stat st;
    if (o.cache_dir && stat(src.path, &st) == 0) {
        key.source_size = (uint64_t)st.st_size;
        key.source_mtime_ns = (int64_t)st.st_mtim.tv_sec * 1000000000ll + st.st_mtim.tv_nsec;
        key.transpose = (uint32_t)transpose;
        keyed = true;
        cpath = std::string(o.cache_dir) + "/" + base_name(src.path) + (transpose ? ".AT" : ".A") + (o.fp32 ? ".f32" : "") + ".pemtile";
        pem_status ls = pem_tiled_load(ctx, cpath.c_str(), &key, out(ctx, *t));
        if (ls == PEM_OK) {
            pem_tiled_info li;
            if (pem_tiled_get_info(t->get(), &li) == PEM_OK && li.value_bytes == (o.fp32 ? 4 : 8)) {
                ++*cache_hits;
                return 0;
            }
            t->reset();   // a file of the other value type under this name: rebuild
            ls = PEM_E_STALE;
        }
        if (ls != PEM_E_IO && ls != PEM_E_STALE) {
            fprintf(stderr, "pemspgemm: %s\n", pem_last_error());
            return 2;
        }
        ++*cache_misses;   // absent, stale or damaged: rebuild below and overwrite
    }
    if (!src.read) {
        if (read_input(o, src.path, &src.coo) != 0) return 1;
        src.read = true;
    }
    if (int rc = convert_or_refuse(ctx, src.path, src.coo, o.fp32, transpose, o.dup, t)) return rc;
    if (keyed && pem_tiled_save(ctx, t->get(), cpath.c_str(), &key) != PEM_OK)
        fprintf(stderr, "pemspgemm: cache not written: %s\n", pem_last_error());   // not fatal
    return 0;
}

// A, B, the mask, the D of --add and of --assign-into, the K of --kron and the F of --hstack / --vstack, the header lines, and the
// conversion time
static int build_operands(const Options &o, pem_ctx *ctx, Operands *in)
{
    auto conv_start = Clock::now();   // spgemm.cu:760: the clock starts before the file is read
    Source srcA = {o.input(), {}, false}, srcB = {o.b_path, {}, false};
    int cache_hits = 0, cache_misses = 0;
    if (int rc = make_tiling(o, ctx, srcA, 0, &in->A, &cache_hits, &cache_misses)) return rc;
    if (o.b_path || o.aat) {
        if (int rc = make_tiling(o, ctx, o.b_path ? srcB : srcA, o.aat ? 1 : 0, &in->B_own, &cache_hits, &cache_misses)) return rc;
    }
    // else the reference converts the same file twice (spgemm.cu:778-779); one tiling serves both roles here
    in->B = in->B_own ? in->B_own.get() : in->A.get();
    pem_tiled_info &ia = in->ia, &ib = in->ib;
    CHECK(pem_tiled_get_info(in->A.get(), &ia));
    CHECK(pem_tiled_get_info(in->B, &ib));
    if (o.sampled_bt) {   // A * B^T from B's rows: the inner dimension is B's columns
        if (ia.cols != ib.cols) {
            printf("inner dimensions differ: A is %d x %d, B^T is %d x %d. Exiting.\n", ia.rows, ia.cols, ib.cols, ib.rows);
            return 1;
        }
    } else if (ia.cols != ib.rows) {
        if (o.b_path)
            printf("inner dimensions differ: A is %d x %d, B%s is %d x %d. Exiting.\n", ia.rows, ia.cols, o.aat ? "^T" : "", ib.rows, ib.cols);
        else
            printf("input is rectangular. Only AAt is possible. Exiting.\n");   // spgemm.cu:782-786
        return 1;
    }
    Coo cm, cd, cinto, ck, cs, csp;
    if (o.sampled_path) {   // S's structure (its values are never read, so it is converted as fp64 whatever --fp32 says)
        if (read_input(o, o.sampled_path, &csp) != 0) return 1;
        const int pcols = o.sampled_bt ? ib.rows : ib.cols;
        if (csp.rows != ia.rows || csp.cols != pcols) {
            printf("--sampled %s is %d x %d but A*B%s is %d x %d. Exiting.\n", o.sampled_path, csp.rows, csp.cols, o.aat || o.sampled_bt ? "^T" : "",
                   ia.rows, pcols);
            return 1;
        }
        if (int rc = convert_or_refuse(ctx, o.sampled_path, csp, false, 0, o.dup, &in->Sp)) return rc;
    }
    if (o.mask_path) {   // M's structure (its values are never read, so it is converted as fp64 whatever --fp32 says)
        if (read_input(o, o.mask_path, &cm) != 0) return 1;
        if (cm.rows != ia.rows || cm.cols != ib.cols) {
            printf("mask %s is %d x %d but C = A*B%s is %d x %d. Exiting.\n", o.mask_path, cm.rows, cm.cols, o.aat ? "^T" : "", ia.rows, ib.cols);
            return 1;
        }
        if (int rc = convert_or_refuse(ctx, o.mask_path, cm, false, 0, o.dup, &in->Mt)) return rc;
    }
    if (o.add_path) {   // D, in the value type of A
        if (read_input(o, o.add_path, &cd) != 0) return 1;
        if (cd.rows != ia.rows || cd.cols != ib.cols) {
            printf("--add %s is %d x %d but C = A*B%s is %d x %d. Exiting.\n", o.add_path, cd.rows, cd.cols, o.aat ? "^T" : "", ia.rows, ib.cols);
            return 1;
        }
        if (int rc = convert_or_refuse(ctx, o.add_path, cd, o.fp32, 0, o.dup, &in->Dt)) return rc;
    }
    if (o.assign_into) {   // D, in the value type of A
        if (read_input(o, o.assign_into, &cinto) != 0) return 1;
        const int dims[2] = {cinto.rows, cinto.cols};
        if (!lists_in_range(assign_flags, o.assign_paths, o.assign_idx, dims, o.assign_into)) return 1;
        if (int rc = convert_or_refuse(ctx, o.assign_into, cinto, o.fp32, 0, o.dup, &in->Into)) return rc;
    }
    if (o.kron_path) {   // K, in the value type of A
        if (read_input(o, o.kron_path, &ck) != 0) return 1;
        if (int rc = convert_or_refuse(ctx, o.kron_path, ck, o.fp32, 0, o.dup, &in->Kt)) return rc;
    }
    if (const char *path = o.stack_paths[0] ? o.stack_paths[0] : o.stack_paths[1]) {   // F, in the value type of A
        if (read_input(o, path, &cs) != 0) return 1;
        if (int rc = convert_or_refuse(ctx, path, cs, o.fp32, 0, o.dup, &in->St)) return rc;
    }
    if (o.fp32) printf("value type: fp32 (the reference computes in fp64)\n");
    printf("MATRIX A\nfilepath: %s\nRows: %d\nCols: %d\nNnz: %lld\n", o.input(), ia.rows, ia.cols, (long long)ia.nnz);   // spgemm.cu:794-806
    printf("MATRIX B\nfilepath: %s\nRows: %d\nCols: %d\nNnz: %lld\n", o.b_path ? o.b_path : o.input(), ib.rows, ib.cols, (long long)ib.nnz);
    if (o.cache_dir) printf("tiled-format cache %s: %d loaded, %d rebuilt\n", o.cache_dir, cache_hits, cache_misses);
    if (o.mask_path)
        printf("MASK%s\nfilepath: %s\nRows: %d\nCols: %d\nNnz: %lld\n", o.mask_complement ? " (complement)" : "", o.mask_path, cm.rows, cm.cols,
               (long long)cm.nnz);
    if (o.sampled_path)
        printf("SAMPLED AT\nfilepath: %s\nRows: %d\nCols: %d\nNnz: %lld\n", o.sampled_path, csp.rows, csp.cols, (long long)csp.nnz);
    in->conv_ms = ms_since(conv_start);
    return 0;
}

// `--power K` computes A^K = (...(A*A)*A...)*A as K-1 products, every C turned into the next left
// operand on the device (pem_tiled_from_cplan), the right operand always A; with --semiring every product uses it.  The first K-2
// products run here, once each.  The timed product is the last one, L * A; its conversion column adds the derived tilings', and
// the report and the CSV row describe it.
static int power_prologue(const Options &o, pem_ctx *ctx, Operands *in, Result *r)
{
    pem_tiled *const A = in->A.get();
    r->L = A;
    for (int k = 2; k < o.power; ++k) {
        uint64_t f = 0;
        CHECK(pem_flop_count(ctx, r->L, A, &f));
        Plan p;
        CHECK(pem_cplan_create(ctx, r->L, A, 0, -1, out(ctx, p)));
        CHECK(pem_cplan_set_semiring(p.get(), o.semiring));
        CHECK(pem_spgemm(ctx, p.get()));
        pem_timings t;
        CHECK(pem_get_timings(ctx, &t));
        Tiled next;
        CHECK(pem_tiled_from_cplan(ctx, p.get(), 0, out(ctx, next)));
        pem_cplan_info pi;
        pem_tiled_info ni;
        CHECK(pem_cplan_get_info(p.get(), &pi));
        CHECK(pem_tiled_get_info(next.get(), &ni));
        printf("power: A^%d = A^%d * A: flop %llu, C nnz %lld, pass %.2fms, C -> operand %.2fms\n", k, k - 1, (unsigned long long)f,
               (long long)pi.nnz_c, t.spgemm_wall_ms, ni.conv_ms);
        in->conv_ms += ni.conv_ms;
        p.reset();
        r->L_own = std::move(next);
        r->L = r->L_own.get();
    }
    return 0;
}

// The plan, WARMUP + REPEAT timed passes of it, the reference's report and the CSV row (22 columns).
static int timed_product(const Options &o, pem_ctx *ctx, const Operands &in, Result *r)
{
    const pem_tiled_info &ia = in.ia, &ib = in.ib;
    pem_tiled_info il;
    CHECK(pem_tiled_get_info(r->L, &il));
    uint64_t flop = 0;
    CHECK(pem_flop_count(ctx, r->L, in.B, &flop));   // spgemm.cu:1068-1079
    if (in.Mt)
        CHECK(pem_cplan_create_masked(ctx, in.A.get(), in.B, in.Mt.get(), o.mask_complement ? PEM_MASK_COMPLEMENT : PEM_MASK_STRUCTURE, 0, -1,
                                      out(ctx, r->plan)));
    else
        CHECK(pem_cplan_create(ctx, r->L, in.B, 0, -1, out(ctx, r->plan)));
    pem_cplan *const plan = r->plan.get();
    CHECK(pem_cplan_set_semiring(plan, o.semiring));
    std::vector<double> s1, s2, s3, wall;
    double cold_ms = 0.0;   // the first pass on the plan: every allocation + the three size read-backs (what the reference pays per iteration)
    for (int n = 0; n < o.WARMUP + o.REPEAT; ++n) {   // spgemm.cu:1133-1357
        if (n == 0) printf("\nstep1 pemSpGEMM (row-local tile-level expand + sort)\n\nstep2 pemSpGEMM\n\nstep3 pemSpGEMM\n\n\n");
        CHECK(pem_spgemm(ctx, plan));
        pem_timings t;
        CHECK(pem_get_timings(ctx, &t));
        if (n == 0) cold_ms = t.spgemm_wall_ms;
        if (n >= o.WARMUP) {
            s1.push_back(t.step1_ms);
            s2.push_back(t.step2_ms);
            s3.push_back(t.step3_ms);
            wall.push_back(t.spgemm_wall_ms);
        }
    }
    auto pick = [&](const std::vector<double> &v, size_t idx) {
        if (v.empty()) return 0.0;
        if (o.fastest) return v[idx];
        return sum_of(v) / (double)v.size();
    };
    size_t fidx = 0;
    if (o.fastest && !wall.empty()) {
        fidx = (size_t)(std::min_element(wall.begin(), wall.end()) - wall.begin());
        printf("fidx: %zu\n\n", fidx);
    } else {
        printf("warm up %d time\naverage over %d iterations\n\n", o.WARMUP, o.REPEAT);
    }
    const double step1 = pick(s1, fidx), step2 = pick(s2, fidx), step3 = pick(s3, fidx), total = pick(wall, fidx);
    const double kernel = step1 + step2 + step3, malloc_ms = total - kernel;   // spgemm.cu:1353-1354
    pem_cplan_info &ci = r->ci;
    CHECK(pem_cplan_get_info(plan, &ci));
    const double gflops = total > 0 ? (double)flop * 2.0 / (total * 1e6) : 0.0;   // spgemm.cu:1403
    const double ratio = ci.nnz_c ? (double)flop / (double)ci.nnz_c : 0.0;       // spgemm.cu:1404

    printf("<---Program done--->\n");   // spgemm.cu:1406-1422
    printf("Matrix A CSR to tile kernel took---------%.2fms\n", ia.conv_tile_kernel_ms);
    printf("Matrix B CSR to tile kernel took---------%.2fms\n", ib.conv_tile_kernel_ms);
    printf("total conversion overhead----------------%.2fms\n\n", in.conv_ms);
    printf("step1 - High Level Multiplication took---%.2fms\n", step1);
    printf("step2 - Allocating C took----------------%.2fms\n", step2);
    printf("step3 - Accumulation took----------------%.2fms\n\n", step3);
    printf("pemSpGEMM took %.2fms ----- GFlops: %.2f\nKernel time %.2fms\nmalloc time %.2fms\n", total, gflops, kernel, malloc_ms);
    printf("first pass (allocations + size read-backs) %.2fms; the passes above re-use the plan's buffers and sizes\n", cold_ms);
    printf("Flop count: %llu\n\n", (unsigned long long)flop);
    if (in.Mt) printf("masked product C<%sM>: the flop count and GFlops above count the unmasked product A*B\n", o.mask_complement ? "!" : "");
    if (o.semiring != PEM_SEMIRING_PLUS_TIMES)
        printf("semiring %s: step 3 reduced under it; the flop count and GFlops above count the tile product's multiply-adds\n", semiring_names[o.semiring]);
    printf("C tiles: %lld\n", (long long)ci.ntiles_c);
    printf("C nnz: %lld\n", (long long)ci.nnz_c);
    if (o.power >= 2)
        printf("power: A^%d = A^%d * A: flop %llu, C nnz %lld, pass %.2fms\n", o.power, o.power - 1, (unsigned long long)flop, (long long)ci.nnz_c, total);
    printf("Compression ratio %.2f\n", ratio);
    // roofline bookkeeping
    const double b_alg = 12.0 * ((double)il.nnz + (double)ib.nnz + (double)ci.nnz_c) + 4.0 * ((double)ia.rows + 1) + 4.0 * ((double)ib.rows + 1) +
                         4.0 * ((double)ia.rows + 1);
    const double frac_kernel = kernel > 0 ? b_alg / (kernel * 1e-3) / 8.0e12 : 0.0, frac_total = total > 0 ? b_alg / (total * 1e-3) / 8.0e12 : 0.0;
    printf("B_alg %.0f bytes; HBM roofline fraction (8 TB/s): kernel %.4f, total %.4f\n", b_alg, frac_kernel, frac_total);

    const pem_csv_record rec = {nullptr, flop, ci.nnz_c, ratio, ia.conv_tile_kernel_ms, ib.conv_tile_kernel_ms, in.conv_ms,
                                step1, step2, step3, total, kernel, malloc_ms, gflops};
    char extra[256];
    // columns 15..: gpus, B_alg, roofline fraction (kernel, total), C tiles, live pairs, first-pass ms, gather ms
    snprintf(extra, sizeof extra, "1,%.0f,%.4f,%.4f,%lld,%lld,%.2f,0.00", b_alg, frac_kernel, frac_total, (long long)ci.ntiles_c, (long long)ci.npairs,
             cold_ms);
    append_csv_row(o, rec, extra);
    return 0;
}

// `--add D.mtx [--alpha x] [--beta y]` computes C = alpha*(A*B) (+) beta*D on the device: the product's
// C becomes a tiling (pem_tiled_from_cplan) and is combined with D over the union of their patterns (pem_tiled_ewise), (+) being
// the semiring's additive op (pem_binop); --out then writes that sum.  D has C's shape and is read with --fp32 like A.
static int add_stage(const Options &o, pem_ctx *ctx, const Operands &in, Result *r)
{
    auto a0 = Clock::now();
    Operand c;
    CHECK(c.open(ctx, *r));
    const int op = add_ops[o.semiring];
    CHECK(pem_tiled_ewise(ctx, c.t, in.Dt.get(), PEM_EWISE_UNION, op, o.add_alpha, o.add_beta, out(ctx, r->sum)));
    const double add_ms = ms_since(a0);
    pem_tiled_info si;
    CHECK(pem_tiled_get_info(r->sum.get(), &si));
    CHECK(pem_tiled_get_info(c.t, &c.info));
    printf("add: C = %g*(A*B) %s %g*D over the union: C -> tiling %.2fms, ewise %.2fms, total %.2fms, nnz %lld\n", o.add_alpha, binop_names[op],
           o.add_beta, c.info.conv_ms, si.conv_ms, add_ms, (long long)si.nnz);
    r->now_last(r->sum, "the sum");
    return 0;
}

// `--apply OP[:THUNK]` changes the values of the final result (C, or the sum of --add) on the device
// (pem_tiled_apply), the pattern kept: OP one of identity abs ainv minv sqrt one (THUNK ignored), plus times min max div rdiv rminus
// (bound to THUNK) or powi (THUNK an integer k in 1..64); THUNK defaults to 0.  Every later stage sees the new tiling.  The CSV row
// describes the product.
static int apply_stage(const Options &o, pem_ctx *ctx, Result *r)
{
    auto a0 = Clock::now();
    Operand src;
    CHECK(src.open(ctx, *r));
    CHECK(pem_tiled_apply(ctx, src.t, o.apply_op, o.apply_thunk, out(ctx, r->app)));
    const double app_total_ms = ms_since(a0);
    pem_tiled_info ai;
    CHECK(pem_tiled_get_info(r->app.get(), &ai));
    printf("apply: %s:%g of %s: apply %.2fms, total %.2fms, nnz %lld\n", apply_names[o.apply_op], o.apply_thunk, r->last_name, ai.conv_ms, app_total_ms,
           (long long)ai.nnz);
    r->now_last(r->app, "the applied matrix");
    return 0;
}

// `--row-scale r.mtx` / `--col-scale c.mtx`, either or both, with `--scale-op OP` (a binop, default
// times): the final result R becomes op(op(r_i, R_ij), c_j) on the device (pem_tiled_scale), the pattern kept.  Each file is a
// Matrix-Market `array real general` file of one column with R.rows resp. R.cols values (read as float with --fp32).  Every later
// stage sees the new tiling.  The CSV row describes the product.
static int scale_stage(const Options &o, pem_ctx *ctx, Result *r)
{
    auto s0 = Clock::now();
    Operand src;
    CHECK(src.open(ctx, *r));
    CHECK(pem_tiled_get_info(src.t, &src.info));
    const int dims[2] = {src.info.rows, src.info.cols};
    DevBuf dv[2];
    for (int q = 0; q < 2; ++q) {
        if (!o.scale_paths[q]) continue;
        if ((long long)o.scale_vec[q].size() != dims[q]) {
            printf("%s %s: the vector has %zu values; the result has %d %s. Exiting.\n", scale_flags[q], o.scale_paths[q], o.scale_vec[q].size(), dims[q],
                   q ? "columns" : "rows");
            return 1;
        }
        if (!dv[q].upload(o.scale_vec[q], o.scale_vec[q].size(), o.fp32)) {
            fprintf(stderr, "pemspgemm: %s: device allocation failed\n", scale_flags[q]);
            return 2;
        }
    }
    CHECK(pem_ctx_synchronize(ctx));
    CHECK(o.fp32 ? pem_tiled_scale_f32(ctx, src.t, o.scale_op, (const float *)dv[0].p, (const float *)dv[1].p, out(ctx, r->scl))
                 : pem_tiled_scale(ctx, src.t, o.scale_op, (const double *)dv[0].p, (const double *)dv[1].p, out(ctx, r->scl)));
    const double scl_total_ms = ms_since(s0);
    pem_tiled_info si;
    CHECK(pem_tiled_get_info(r->scl.get(), &si));
    printf("scale: %s of %s by %s%s%s: scale %.2fms, total %.2fms, nnz %lld\n", binop_names[o.scale_op], r->last_name, o.scale_paths[0] ? "rows" : "",
           o.scale_paths[0] && o.scale_paths[1] ? " and " : "", o.scale_paths[1] ? "columns" : "", si.conv_ms, scl_total_ms, (long long)si.nnz);
    r->now_last(r->scl, "the scaled matrix");
    return 0;
}

// `--select OP[:THUNK]` keeps the entries of the final result (C, or the sum of --add) that satisfy
// OP, one of tril triu diag offdiag row_le row_gt col_le col_gt (THUNK an integer k) or value_eq value_ne value_lt value_le
// value_gt value_ge abs_gt (THUNK a value); THUNK defaults to 0.  The result becomes a tiling (pem_tiled_from_cplan, or the
// ewise sum) and is filtered on the device (pem_tiled_select); --out then writes what is kept.  The CSV row describes the product.
static int select_stage(const Options &o, pem_ctx *ctx, Result *r)
{
    auto s0 = Clock::now();
    Operand src;
    CHECK(src.open(ctx, *r));
    CHECK(pem_tiled_select(ctx, src.t, o.select_op, o.select_thunk, out(ctx, r->sel)));
    const double sel_total_ms = ms_since(s0);
    pem_tiled_info si;
    CHECK(pem_tiled_get_info(r->sel.get(), &si));
    CHECK(pem_tiled_get_info(src.t, &src.info));
    printf("select: %s:%g of %s: select %.2fms, total %.2fms, nnz %lld of %lld kept\n", select_names[o.select_op], o.select_thunk, r->last_name,
           si.conv_ms, sel_total_ms, (long long)si.nnz, (long long)src.info.nnz);
    r->now_last(r->sel, "the selection");
    return 0;
}

// `--topk DIM:ORDER:K` keeps, of every row (DIM rows) or column (cols) of the final result (C, the sum
// of --add, what --apply / --row/col-scale changed or --select kept), the first K entries in rank order: ORDER one of largest
// smallest abs_largest, NaNs last, ties by ascending index (pem_tiled_select_topk).  Every later stage sees the new tiling.  The
// CSV row describes the product.
static int topk_stage(const Options &o, pem_ctx *ctx, Result *r)
{
    auto s0 = Clock::now();
    Operand src;
    CHECK(src.open(ctx, *r));
    CHECK(pem_tiled_select_topk(ctx, src.t, o.topk_order, o.topk_dim, (int64_t)o.topk_k, out(ctx, r->top)));
    const double top_total_ms = ms_since(s0);
    pem_tiled_info ti;
    CHECK(pem_tiled_get_info(r->top.get(), &ti));
    CHECK(pem_tiled_get_info(src.t, &src.info));
    printf("topk: %s:%s:%lld of %s: topk %.2fms, total %.2fms, nnz %lld of %lld kept\n", dim_names[o.topk_dim], topk_names[o.topk_order], o.topk_k,
           r->last_name, ti.conv_ms, top_total_ms, (long long)ti.nnz, (long long)src.info.nnz);
    r->now_last(r->top, "the top-k selection");
    return 0;
}

// `--extract-rows I.mtx` / `--extract-cols J.mtx`, either or both: the final result R (C, the sum of
// --add, or what --select kept) becomes R(I, J) on the device (pem_tiled_extract).  Each file is a Matrix-Market `array` file of
// one column holding 1-based indices (`integer`, or `real` with integral values), in any order, repeats allowed.  --reduce,
// --spmm, --sddmm and --out then see the extracted tiling.  The CSV row describes the product.
static int extract_stage(const Options &o, pem_ctx *ctx, Result *r)
{
    auto x0 = Clock::now();
    Operand src;
    CHECK(src.open(ctx, *r));
    CHECK(pem_tiled_get_info(src.t, &src.info));
    const int dims[2] = {src.info.rows, src.info.cols};
    if (!lists_in_range(extract_flags, o.extract_paths, o.extract_idx, dims, "the result")) return 1;
    CHECK(pem_tiled_extract(ctx, src.t, o.extract_paths[0] ? o.extract_idx[0].data() : nullptr, (int64_t)o.extract_idx[0].size(),
                            o.extract_paths[1] ? o.extract_idx[1].data() : nullptr, (int64_t)o.extract_idx[1].size(), out(ctx, r->ext)));
    const double ext_total_ms = ms_since(x0);
    pem_tiled_info xi;
    CHECK(pem_tiled_get_info(r->ext.get(), &xi));
    printf("extract: %s x %s of %s: extract %.2fms, total %.2fms, %d x %d, nnz %lld from %lld\n",
           count_or_all(o.extract_paths[0], o.extract_idx[0].size(), "rows").c_str(),
           count_or_all(o.extract_paths[1], o.extract_idx[1].size(), "columns").c_str(), r->last_name, xi.conv_ms, ext_total_ms, xi.rows, xi.cols,
           (long long)xi.nnz, (long long)src.info.nnz);
    r->now_last(r->ext, "the extract");
    return 0;
}

// `--assign-into D.mtx [--assign-rows I.mtx] [--assign-cols J.mtx] [--assign-accum OP]`: after the
// product and any --add / --select / --extract-*, the final result R is written into D at (I, J) on the device (pem_tiled_assign):
// D(I, J) = R, or D(I, J) = OP(D(I, J), R) with OP one of plus times min max lor land.  The lists are files like --extract-rows'
// (1-based, any order, no repeats; absent = all); R must be |I| x |J|.  D is read with --fp32 like A.  --reduce, --spmm, --sddmm,
// --out and the sorted COO files then see that tiling.  The CSV row describes the product.
static int assign_stage(const Options &o, pem_ctx *ctx, const Operands &in, Result *r)
{
    auto g0 = Clock::now();
    Operand src;
    CHECK(src.open(ctx, *r));
    pem_tiled_info gi, di;
    CHECK(pem_tiled_get_info(src.t, &src.info));
    CHECK(pem_tiled_get_info(in.Into.get(), &di));
    const long long want_r = o.assign_paths[0] ? (long long)o.assign_idx[0].size() : di.rows;
    const long long want_c = o.assign_paths[1] ? (long long)o.assign_idx[1].size() : di.cols;
    if (src.info.rows != want_r || src.info.cols != want_c) {
        printf("--assign-into %s: the result is %d x %d but the region is %lld x %lld (%s is %d x %d). Exiting.\n", o.assign_into, src.info.rows,
               src.info.cols, want_r, want_c, o.assign_into, di.rows, di.cols);
        return 1;
    }
    CHECK(pem_tiled_assign(ctx, in.Into.get(), src.t, o.assign_paths[0] ? o.assign_idx[0].data() : nullptr, (int64_t)o.assign_idx[0].size(),
                           o.assign_paths[1] ? o.assign_idx[1].data() : nullptr, (int64_t)o.assign_idx[1].size(), o.assign_accum, out(ctx, r->asg)));
    const double asg_total_ms = ms_since(g0);
    CHECK(pem_tiled_get_info(r->asg.get(), &gi));
    const bool accum = o.assign_accum != PEM_ACCUM_NONE;
    printf("assign: %s into %s at %s x %s%s%s: assign %.2fms, total %.2fms, %d x %d, nnz %lld (D %lld, the result %lld)\n", r->last_name, o.assign_into,
           count_or_all(o.assign_paths[0], o.assign_idx[0].size(), "rows").c_str(),
           count_or_all(o.assign_paths[1], o.assign_idx[1].size(), "columns").c_str(), accum ? ", accum " : "", accum ? binop_names[o.assign_accum] : "",
           gi.conv_ms, asg_total_ms, gi.rows, gi.cols, (long long)gi.nnz, (long long)di.nnz, (long long)src.info.nnz);
    r->now_last(r->asg, "the assigned matrix");
    return 0;
}

// `--kron K.mtx [--kron-op OP]`: after the product and every stage above, the final result R becomes
// R (x) K on the device (pem_tiled_kron): R.rows * K.rows by R.cols * K.cols, entry (i * K.rows + k, j * K.cols + l) = OP(r_ij, k_kl)
// with OP one of plus times min max lor land (default times, the Kronecker product proper).  K is read with --fp32 like A.
// --reduce, --bfs, --spmm, --sddmm, --out and the sorted COO files then see that tiling.  A result whose dimensions or entries leave
// the int32 range is refused with the library's message.  The CSV row describes the product.
static int kron_stage(const Options &o, pem_ctx *ctx, const Operands &in, Result *r)
{
    auto k0 = Clock::now();
    Operand src;
    CHECK(src.open(ctx, *r));
    const pem_status s = pem_tiled_kron(ctx, src.t, in.Kt.get(), o.kron_op, out(ctx, r->krn));
    if (s == PEM_E_OVERFLOW) {
        printf("--kron %s: %s. Exiting.\n", o.kron_path, pem_last_error());
        return 1;
    }
    CHECK(s);
    const double krn_total_ms = ms_since(k0);
    pem_tiled_info ki, kk;
    CHECK(pem_tiled_get_info(r->krn.get(), &ki));
    CHECK(pem_tiled_get_info(in.Kt.get(), &kk));
    CHECK(pem_tiled_get_info(src.t, &src.info));
    printf("kron: %s (x) %s under %s: kron %.2fms, total %.2fms, %d x %d, nnz %lld (the result %lld, K %lld)\n", r->last_name, o.kron_path,
           binop_names[o.kron_op], ki.conv_ms, krn_total_ms, ki.rows, ki.cols, (long long)ki.nnz, (long long)src.info.nnz, (long long)kk.nnz);
    r->now_last(r->krn, "the Kronecker product");
    return 0;
}

// `--hstack F.mtx` / `--vstack F.mtx`: after the product and every stage above, the final result R becomes
// [R F] resp. [R; F] on the device (pem_tiled_concat, a 1 x 2 resp. 2 x 1 grid).  F is read with --fp32 like A and must have R's row
// resp. column count.  --reduce, --bfs, --spmm, --sddmm, --out and the sorted COO files then see that tiling.  The CSV row describes
// the product.
static int stack_stage(const Options &o, pem_ctx *ctx, const Operands &in, Result *r)
{
    const int v = o.stack_paths[1] ? 1 : 0;
    auto s0 = Clock::now();
    Operand src;
    CHECK(src.open(ctx, *r));
    pem_tiled_info fi;
    CHECK(pem_tiled_get_info(src.t, &src.info));
    CHECK(pem_tiled_get_info(in.St.get(), &fi));
    if (v ? fi.cols != src.info.cols : fi.rows != src.info.rows) {
        printf("%s %s is %d x %d but %s is %d x %d: the %s counts differ. Exiting.\n", stack_flags[v], o.stack_paths[v], fi.rows, fi.cols,
               r->last_name, src.info.rows, src.info.cols, v ? "column" : "row");
        return 1;
    }
    const pem_tiled *const blocks[2] = {src.t, in.St.get()};
    const int64_t own_rows[2] = {src.info.rows, fi.rows}, own_cols[2] = {src.info.cols, fi.cols};
    const pem_status s = v ? pem_tiled_concat(ctx, 2, 1, blocks, own_rows, own_cols, out(ctx, r->stk))
                           : pem_tiled_concat(ctx, 1, 2, blocks, own_rows, own_cols, out(ctx, r->stk));
    if (s == PEM_E_OVERFLOW) {
        printf("%s %s: %s. Exiting.\n", stack_flags[v], o.stack_paths[v], pem_last_error());
        return 1;
    }
    CHECK(s);
    const double stk_total_ms = ms_since(s0);
    pem_tiled_info si;
    CHECK(pem_tiled_get_info(r->stk.get(), &si));
    printf("%s: [%s%s %s]: concat %.2fms, total %.2fms, %d x %d, nnz %lld (the result %lld, F %lld)\n", stack_flags[v] + 2, r->last_name, v ? ";" : "",
           o.stack_paths[v], si.conv_ms, stk_total_ms, si.rows, si.cols, (long long)si.nnz, (long long)src.info.nnz, (long long)fi.nnz);
    r->now_last(r->stk, "the stacked matrix");
    return 0;
}

// `--reduce rows|cols[:OP]` folds every row or column of the final result (C, the sum of --add, or
// what --select kept) on the device (pem_tiled_reduce); OP is one of plus times min max lor land and defaults to the semiring's
// additive op.  --out then writes the vector (Matrix-Market array) instead of the matrix.  The CSV row describes the product.
static int reduce_stage(const Options &o, pem_ctx *ctx, Result *r)
{
    Operand src;
    CHECK(src.open(ctx, *r));
    CHECK(pem_tiled_get_info(src.t, &src.info));
    const size_t n = (size_t)(o.reduce_dim == PEM_REDUCE_COLS ? src.info.cols : src.info.rows);
    DevBuf dy;
    if (!dy.alloc(n, o.fp32 ? 4 : 8)) {
        fprintf(stderr, "pemspgemm: --reduce: device allocation of %zu values failed\n", n);
        return 2;
    }
    CHECK(pem_ctx_synchronize(ctx));
    auto r0 = Clock::now();
    CHECK(o.fp32 ? pem_tiled_reduce_f32(ctx, src.t, o.reduce_op, o.reduce_dim, (float *)dy.p, 0)
                 : pem_tiled_reduce(ctx, src.t, o.reduce_op, o.reduce_dim, (double *)dy.p, 0));
    CHECK(pem_ctx_synchronize(ctx));
    const double red_ms = ms_since(r0);
    if (!dy.download(&r->red, n, o.fp32)) return 2;
    printf("reduce: %s %s of %s: reduce %.3fms, %zu values, host sum %.17g\n", o.reduce_dim == PEM_REDUCE_COLS ? "cols" : "rows",
           binop_names[o.reduce_op], r->last_name, red_ms, n, sum_of(r->red));
    return 0;
}

// `--ilu0` replaces the final result (C, or what --add, --select, --apply ... left) by its incomplete LU
// on its own pattern (pem_tiled_ilu0): L's strict lower triangle and U in one tiling.  It is the last matrix stage: the vector
// stages see the factor, so `--ilu0 --trsv lower:unit --rhs b.mtx` applies L^-1, and --out writes F.  The result must be square and
// store every diagonal entry.  The CSV row describes the product.
static int ilu0_stage(const Options &, pem_ctx *ctx, Result *r)
{
    auto t0 = Clock::now();
    Operand src;
    CHECK(src.open(ctx, *r));
    pem_tiled_info si;
    CHECK(pem_tiled_get_info(src.t, &si));
    if (si.rows != si.cols) {
        printf("--ilu0: %s is %d x %d; an incomplete LU needs a square matrix. Exiting.\n", r->last_name, si.rows, si.cols);
        return 1;
    }
    if (pem_tiled_ilu0(ctx, src.t, out(ctx, r->ilu)) != PEM_OK) {
        printf("--ilu0: %s. Exiting.\n", pem_last_error());
        return 1;
    }
    const double total_ms = ms_since(t0);
    pem_tiled_info fi;
    CHECK(pem_tiled_get_info(r->ilu.get(), &fi));
    pem_ilu0_info ii;
    CHECK(pem_tiled_ilu0_info(ctx, r->ilu.get(), &ii));
    printf("ilu0: of %s: ilu0 %.2fms, total %.2fms, nnz %lld, %lld levels, %lld launches, %lld zero pivots\n", r->last_name, fi.conv_ms, total_ms,
           (long long)fi.nnz, (long long)ii.levels, (long long)ii.launches, (long long)ii.zero_pivots);
    r->now_last(r->ilu, "the ILU(0) factor");
    return 0;
}

// `--trsv lower|upper[:unit] [--rhs b.mtx]` solves T x = b on the device (pem_tiled_trsv), T the named
// triangle of the final result (what --reduce would fold; it must be square) as stored, the diagonal taken as 1 under :unit.  b is
// a Matrix-Market `array real general` file of one column, all ones without --rhs.  One line reports the solve's time (the
// schedule built by a first solve, which is timed apart), the levels and the launches; --out then writes x (Matrix-Market array)
// instead of the matrix.  The CSV row describes the product.
static int trsv_stage(const Options &o, pem_ctx *ctx, Result *r)
{
    Operand src;
    CHECK(src.open(ctx, *r));
    const pem_tiled_info &si = src.info;
    CHECK(pem_tiled_get_info(src.t, &src.info));
    if (si.rows != si.cols) {
        printf("--trsv %s: %s is %d x %d; a triangular solve needs a square matrix. Exiting.\n", o.trsv_spec, r->last_name, si.rows, si.cols);
        return 1;
    }
    const size_t n = (size_t)si.rows;
    if (o.rhs_path && o.rhs.size() != n) {
        printf("--rhs %s: the vector has %zu values; %s has %d rows. Exiting.\n", o.rhs_path, o.rhs.size(), r->last_name, si.rows);
        return 1;
    }
    const std::vector<double> ones(o.rhs_path ? 0 : n, 1.0);
    DevBuf db, dx;
    if (!db.upload(o.rhs_path ? o.rhs : ones, n, o.fp32) || !dx.alloc(n, o.fp32 ? 4 : 8)) {
        fprintf(stderr, "pemspgemm: --trsv: device allocation of %zu values failed\n", n);
        return 2;
    }
    const auto solve = [&] {
        return o.fp32 ? pem_tiled_trsv_f32(ctx, src.t, o.trsv_uplo, o.trsv_unit, (const float *)db.p, (float *)dx.p)
                      : pem_tiled_trsv(ctx, src.t, o.trsv_uplo, o.trsv_unit, (const double *)db.p, (double *)dx.p);
    };
    CHECK(pem_ctx_synchronize(ctx));
    auto t0 = Clock::now();
    const pem_status first = solve();   // builds the schedule
    if (first == PEM_E_INVALID) {
        printf("--trsv %s: %s. Exiting.\n", o.trsv_spec, pem_last_error());
        return 1;
    }
    CHECK(first);
    CHECK(pem_ctx_synchronize(ctx));
    const double first_ms = ms_since(t0);
    t0 = Clock::now();
    CHECK(solve());
    CHECK(pem_ctx_synchronize(ctx));
    const double solve_ms = ms_since(t0);
    pem_trsv_info ti;
    CHECK(pem_tiled_trsv_info(ctx, src.t, o.trsv_uplo, &ti));
    if (!dx.download(&r->trsv_x, n, o.fp32)) return 2;
    printf("trsv: %s%s of %s: solve %.3fms (first, with the schedule, %.3fms), %zu values, %lld levels, %lld launches, host sum %.17g\n",
           o.trsv_uplo == PEM_TRSV_UPPER ? "upper" : "lower", o.trsv_unit ? ":unit" : "", r->last_name, solve_ms, first_ms, n, (long long)ti.levels,
           (long long)ti.launches, sum_of(r->trsv_x));
    return 0;
}

// `--solve cg|bicgstab --rhs b.mtx [--precond none|jacobi|ilu0 | --amg smoothed|plain] [--rtol R] [--max-iters N]` (INTEGRATION.md
// sections 3zc, 3zd) solves
// R x = b on the device (pem_krylov_*), R the final result (what --reduce would fold; it must be square), from a zero guess.
// jacobi: the inverse of R's diagonal (pem_tiled_select + pem_tiled_reduce, inverted on the host in the value type); ilu0: the
// stage's own pem_tiled_ilu0(R); --amg: the stage's own pem_amg_create(R) with the defaults of the Python binding's Amg (symmetric
// = 0, seed 0, 16 levels, coarse_size 40, one sweep, four coarse sweeps, omega 2/3, not refreshable), reported on an `amg:` line --
// levels, rows level by level, the operator complexity sum nnz(A_l) / nnz(A_0), setup ms.  One line reports the time, the iterations, the status and sqrt(rr / bb); --out then writes x
// (Matrix-Market array) instead of the matrix.  A status other than converged is reported, not refused.  The CSV row describes the
// product.
static int solve_stage(const Options &o, pem_ctx *ctx, Result *r)
{
    Operand src;
    CHECK(src.open(ctx, *r));
    const pem_tiled_info &si = src.info;
    CHECK(pem_tiled_get_info(src.t, &src.info));
    if (si.rows != si.cols) {
        printf("--solve %s: %s is %d x %d; a Krylov solver needs a square matrix. Exiting.\n", o.solve_spec, r->last_name, si.rows, si.cols);
        return 1;
    }
    const size_t n = (size_t)si.rows;
    if (o.rhs.size() != n) {
        printf("--rhs %s: the vector has %zu values; %s has %d rows. Exiting.\n", o.rhs_path, o.rhs.size(), r->last_name, si.rows);
        return 1;
    }
    const std::vector<double> zeros(n, 0.0);
    DevBuf db, dx, dm;
    if (!db.upload(o.rhs, n, o.fp32) || !dx.upload(zeros, n, o.fp32)) {
        fprintf(stderr, "pemspgemm: --solve: device allocation of %zu values failed\n", n);
        return 2;
    }
    CHECK(pem_ctx_synchronize(ctx));
    auto t0 = Clock::now();
    Tiled F;
    if (o.solve_precond == 1) {
        Tiled D;
        CHECK(pem_tiled_select(ctx, src.t, PEM_SELECT_DIAG, 0.0, out(ctx, D)));
        if (!dm.alloc(n, o.fp32 ? 4 : 8)) return 2;
        CHECK(o.fp32 ? pem_tiled_reduce_f32(ctx, D.get(), PEM_BINOP_PLUS, PEM_REDUCE_ROWS, (float *)dm.p, 0)
                     : pem_tiled_reduce(ctx, D.get(), PEM_BINOP_PLUS, PEM_REDUCE_ROWS, (double *)dm.p, 0));
        CHECK(pem_ctx_synchronize(ctx));
        std::vector<double> d;
        if (!dm.download(&d, n, o.fp32)) return 2;
        for (double &v : d) v = o.fp32 ? (double)(1.0f / (float)v) : 1.0 / v;
        DevBuf inv;
        if (!inv.upload(d, n, o.fp32)) return 2;
        std::swap(dm.p, inv.p);
    } else if (o.solve_precond == 2) {
        if (pem_tiled_ilu0(ctx, src.t, out(ctx, F)) != PEM_OK) {
            printf("--precond ilu0: %s. Exiting.\n", pem_last_error());
            return 1;
        }
    }
    struct AmgHandle {
        pem_ctx *ctx;
        pem_amg *M = nullptr;
        ~AmgHandle() { pem_amg_destroy(ctx, M); }
    } amg{ctx};
    if (o.amg_smooth >= 0) {
        pem_amg_opts ao;
        ao.smooth = o.amg_smooth;
        ao.symmetric = 0;
        ao.seed = 0;
        ao.max_levels = PEM_AMG_MAX_LEVELS;
        ao.coarse_size = 40;
        ao.sweeps = 1;
        ao.coarse_sweeps = 4;
        ao.omega = 2.0 / 3.0;
        ao.refreshable = 0;
        if (pem_amg_create(ctx, src.t, &ao, &amg.M) != PEM_OK) {
            printf("--amg %s: %s. Exiting.\n", o.amg_kind, pem_last_error());
            return 1;
        }
    }
    const double setup_ms = ms_since(t0);
    if (amg.M) {
        pem_amg_info ai;
        CHECK(pem_amg_get_info(amg.M, &ai));
        std::string rows;
        int64_t nnz_all = 0;
        for (int l = 0; l < ai.levels; ++l) {
            rows += (l ? ", " : "") + std::to_string((long long)ai.rows[l]);
            nnz_all += ai.nnz[l];
        }
        printf("amg: %s of %s: %d levels, rows %s, operator complexity %.4f, %lld launches per cycle, setup %.3fms\n", o.amg_kind, r->last_name,
               (int)ai.levels, rows.c_str(), ai.nnz[0] ? (double)nnz_all / (double)ai.nnz[0] : 1.0, (long long)ai.launches, setup_ms);
    }
    pem_krylov_opts ko;
    ko.method = o.solve_method;
    ko.precond = amg.M ? (int)PEM_PRECOND_AMG : o.solve_precond == 1 ? PEM_PRECOND_DIAG : o.solve_precond == 2 ? PEM_PRECOND_LU : PEM_PRECOND_NONE;
    ko.max_iters = o.solve_max_iters;
    ko.check_every = 8;
    ko.rtol = o.solve_rtol;
    ko.atol = 0.0;
    pem_krylov *K = nullptr;
    if ((amg.M ? pem_krylov_create_amg(ctx, src.t, &ko, amg.M, &K) : pem_krylov_create(ctx, src.t, &ko, F.get(), &K)) != PEM_OK) {
        printf("--solve %s: %s. Exiting.\n", o.solve_spec, pem_last_error());
        return 1;
    }
    pem_krylov_result res;
    t0 = Clock::now();
    const pem_status st = o.fp32 ? pem_krylov_solve_f32(ctx, K, (const float *)db.p, (float *)dx.p, (const float *)dm.p, nullptr, &res)
                                 : pem_krylov_solve(ctx, K, (const double *)db.p, (double *)dx.p, (const double *)dm.p, nullptr, &res);
    const double solve_ms = ms_since(t0);
    pem_krylov_destroy(ctx, K);
    CHECK(st);
    if (!dx.download(&r->solve_x, n, o.fp32)) return 2;
    static const char *const status[] = {"converged", "max_iters", "breakdown", "nonfinite"};
    printf("solve: %s with %s of %s: solve %.3fms (preconditioner %.3fms), %lld iterations, %s, relative residual %.3e, %lld read-backs, host sum %.17g\n",
           o.solve_spec, amg.M ? "amg" : o.precond_name ? o.precond_name : "none", r->last_name, solve_ms, setup_ms, (long long)res.iters, status[res.status],
           sqrt(res.rr / res.bb), (long long)res.readbacks, sum_of(r->solve_x));
    return 0;
}

// `--bfs SRC` runs a breadth-first search from the 1-based vertex SRC over the pattern of the final
// result (what --reduce would fold; it must be square) on the device (pem_tiled_bfs): a stored entry (i, j) is an edge i -> j.
// One line reports depth, reached and the time; --out then writes the levels (Matrix-Market `array integer general`, -1 for
// unreachable) instead of the matrix.  The CSV row describes the product.
static int bfs_stage(const Options &o, pem_ctx *ctx, Result *r)
{
    Operand src;
    CHECK(src.open(ctx, *r));
    const pem_tiled_info &si = src.info;
    CHECK(pem_tiled_get_info(src.t, &src.info));
    if (si.rows != si.cols) {
        printf("--bfs %s: %s is %d x %d; a search needs a square matrix. Exiting.\n", o.bfs_spec, r->last_name, si.rows, si.cols);
        return 1;
    }
    if (o.bfs_src > si.rows) {
        printf("--bfs %s: %s has %d vertices. Exiting.\n", o.bfs_spec, r->last_name, si.rows);
        return 1;
    }
    const size_t n = (size_t)si.rows;
    DevBuf dl;
    if (!dl.alloc(n, 4)) {
        fprintf(stderr, "pemspgemm: --bfs: device allocation of %zu levels failed\n", n);
        return 2;
    }
    CHECK(pem_ctx_synchronize(ctx));
    int32_t depth = 0;
    int64_t reached = 0;
    auto b0 = Clock::now();
    CHECK(pem_tiled_bfs(ctx, src.t, (int64_t)(o.bfs_src - 1), 0, (int32_t *)dl.p, &depth, &reached));
    const double bfs_ms = ms_since(b0);
    std::vector<int32_t> levels(n);
    if (hipMemcpy(levels.data(), dl.p, 4 * n, hipMemcpyDeviceToHost) != hipSuccess) return 2;
    r->bfs_levels.assign(levels.begin(), levels.end());
    printf("bfs: from %lld over %s: depth %d, reached %lld of %zu, bfs %.3fms\n", o.bfs_src, r->last_name, depth, (long long)reached, n, bfs_ms);
    return 0;
}

// `--argreduce rows|cols:min|max` finds, for every row or column of the final result (what --reduce
// would fold), where its minimum or maximum sits, on the device (pem_tiled_reduce_arg): the smallest index inside the line whose
// stored value equals the fold.  One line reports the time; --out then writes the indices (Matrix-Market `array integer general`,
// 1-based, 0 where the line has no non-NaN entry) instead of the matrix.  The CSV row describes the product.
static int argreduce_stage(const Options &o, pem_ctx *ctx, Result *r)
{
    Operand src;
    CHECK(src.open(ctx, *r));
    CHECK(pem_tiled_get_info(src.t, &src.info));
    const size_t n = (size_t)(o.argreduce_dim == PEM_REDUCE_COLS ? src.info.cols : src.info.rows);
    DevBuf dy, di;
    if (!dy.alloc(n, o.fp32 ? 4 : 8) || !di.alloc(n, 4)) {
        fprintf(stderr, "pemspgemm: --argreduce: device allocation of %zu values and indices failed\n", n);
        return 2;
    }
    CHECK(pem_ctx_synchronize(ctx));
    auto r0 = Clock::now();
    CHECK(o.fp32 ? pem_tiled_reduce_arg_f32(ctx, src.t, o.argreduce_op, o.argreduce_dim, (float *)dy.p, (int32_t *)di.p)
                 : pem_tiled_reduce_arg(ctx, src.t, o.argreduce_op, o.argreduce_dim, (double *)dy.p, (int32_t *)di.p));
    CHECK(pem_ctx_synchronize(ctx));
    const double arg_ms = ms_since(r0);
    std::vector<int32_t> idx(n);
    if (n && hipMemcpy(idx.data(), di.p, 4 * n, hipMemcpyDeviceToHost) != hipSuccess) return 2;
    r->arg_idx.resize(n);
    size_t found = 0;
    for (size_t i = 0; i < n; ++i) {
        r->arg_idx[i] = (double)(idx[i] + 1);
        found += idx[i] >= 0;
    }
    printf("argreduce: %s %s of %s: argreduce %.3fms, %zu indices, %zu lines with one\n", o.argreduce_dim == PEM_REDUCE_COLS ? "cols" : "rows",
           binop_names[o.argreduce_op], r->last_name, arg_ms, n, found);
    return 0;
}

// `--bfs-parents SRC` is --bfs with the breadth-first tree (pem_tiled_bfs_parents): the line --bfs
// prints, and --out writes the parents (Matrix-Market `array integer general`, 1-based, SRC its own parent, 0 where the vertex is
// unreachable) instead of the matrix.  The CSV row describes the product.
static int bfs_parents_stage(const Options &o, pem_ctx *ctx, Result *r)
{
    Operand src;
    CHECK(src.open(ctx, *r));
    const pem_tiled_info &si = src.info;
    CHECK(pem_tiled_get_info(src.t, &src.info));
    if (si.rows != si.cols) {
        printf("--bfs-parents %s: %s is %d x %d; a search needs a square matrix. Exiting.\n", o.bfs_parents_spec, r->last_name, si.rows, si.cols);
        return 1;
    }
    if (o.bfs_parents_src > si.rows) {
        printf("--bfs-parents %s: %s has %d vertices. Exiting.\n", o.bfs_parents_spec, r->last_name, si.rows);
        return 1;
    }
    const size_t n = (size_t)si.rows;
    DevBuf dl, dp;
    if (!dl.alloc(n, 4) || !dp.alloc(n, 4)) {
        fprintf(stderr, "pemspgemm: --bfs-parents: device allocation of %zu levels and parents failed\n", n);
        return 2;
    }
    CHECK(pem_ctx_synchronize(ctx));
    int32_t depth = 0;
    int64_t reached = 0;
    auto b0 = Clock::now();
    CHECK(pem_tiled_bfs_parents(ctx, src.t, (int64_t)(o.bfs_parents_src - 1), 0, (int32_t *)dl.p, (int32_t *)dp.p, &depth, &reached));
    const double bfs_ms = ms_since(b0);
    std::vector<int32_t> parents(n);
    if (hipMemcpy(parents.data(), dp.p, 4 * n, hipMemcpyDeviceToHost) != hipSuccess) return 2;
    r->bfs_parents.resize(n);
    for (size_t v = 0; v < n; ++v) r->bfs_parents[v] = (double)(parents[v] + 1);
    printf("bfs: from %lld over %s: depth %d, reached %lld of %zu, bfs %.3fms\n", o.bfs_parents_src, r->last_name, depth, (long long)reached, n,
           bfs_ms);
    return 0;
}

// `--colour SEED` / `--colour-natural` colours the graph of the final result's pattern (what --reduce
// would fold; it must be square; every stored off-diagonal entry is an undirected edge) on the device (pem_tiled_colour): the greedy
// colouring in the order of the priorities SEED hashes, or in natural order (equal priorities).  One line reports colours, rounds
// and the time; --out then writes the colours (Matrix-Market `array integer general`, 1-based) instead of the matrix.  The CSV
// row describes the product.
static int colour_stage(const Options &o, pem_ctx *ctx, Result *r)
{
    Operand src;
    CHECK(src.open(ctx, *r));
    const pem_tiled_info &si = src.info;
    CHECK(pem_tiled_get_info(src.t, &src.info));
    if (si.rows != si.cols) {
        printf("%s: %s is %d x %d; a colouring needs a square matrix. Exiting.\n", o.colour_flag(), r->last_name, si.rows, si.cols);
        return 1;
    }
    const size_t n = (size_t)si.rows;
    DevBuf dc, dp;
    if (!dc.alloc(n, 4) || (o.colour_natural && !dp.alloc(n, 4))) {
        fprintf(stderr, "pemspgemm: %s: device allocation of %zu colours failed\n", o.colour_flag(), n);
        return 2;
    }
    // (the fill runs on the null stream, the colouring on the context's: wait for it)
    if (o.colour_natural && n && (hipMemset(dp.p, 0, 4 * n) != hipSuccess || hipDeviceSynchronize() != hipSuccess)) return 2;
    CHECK(pem_ctx_synchronize(ctx));
    int32_t ncolours = 0, rounds = 0;
    auto c0 = Clock::now();
    CHECK(pem_tiled_colour(ctx, src.t, 0, o.colour_seed, o.colour_natural ? (const uint32_t *)dp.p : nullptr, (int32_t *)dc.p, &ncolours, &rounds));
    const double colour_ms = ms_since(c0);
    std::vector<int32_t> colours(n);
    if (n && hipMemcpy(colours.data(), dc.p, 4 * n, hipMemcpyDeviceToHost) != hipSuccess) return 2;
    r->colours.resize(n);
    for (size_t v = 0; v < n; ++v) r->colours[v] = (double)(colours[v] + 1);
    printf("colour: %s of %s: %d colours in %d rounds, %zu vertices, colour %.3fms\n",
           o.colour_natural ? "natural order" : (std::string("seed ") + o.colour_spec).c_str(), r->last_name, ncolours, rounds, n, colour_ms);
    return 0;
}

// `--components` labels the connected components of the graph of the final result's pattern (what
// --colour would colour; it must be square; every stored entry is an undirected edge, stored one way or both) on the device
// (pem_tiled_components): every vertex gets the smallest vertex of its component.  One line reports components, rounds and the
// time; --out then writes the labels (Matrix-Market `array integer general`, 1-based) instead of the matrix.  The CSV row describes
// the product.
static int components_stage(const Options &, pem_ctx *ctx, Result *r)
{
    Operand src;
    CHECK(src.open(ctx, *r));
    const pem_tiled_info &si = src.info;
    CHECK(pem_tiled_get_info(src.t, &src.info));
    if (si.rows != si.cols) {
        printf("--components: %s is %d x %d; the components need a square matrix. Exiting.\n", r->last_name, si.rows, si.cols);
        return 1;
    }
    const size_t n = (size_t)si.rows;
    DevBuf dl;
    if (!dl.alloc(n, 4)) {
        fprintf(stderr, "pemspgemm: --components: device allocation of %zu labels failed\n", n);
        return 2;
    }
    CHECK(pem_ctx_synchronize(ctx));
    int64_t ncomponents = 0;
    int32_t rounds = 0;
    auto c0 = Clock::now();
    CHECK(pem_tiled_components(ctx, src.t, 0, (int32_t *)dl.p, nullptr, &ncomponents, &rounds));
    const double components_ms = ms_since(c0);
    std::vector<int32_t> labels(n);
    if (n && hipMemcpy(labels.data(), dl.p, 4 * n, hipMemcpyDeviceToHost) != hipSuccess) return 2;
    r->labels.resize(n);
    for (size_t v = 0; v < n; ++v) r->labels[v] = (double)(labels[v] + 1);
    printf("components: %lld components in %d rounds, %zu vertices, %.3fms\n", (long long)ncomponents, rounds, n, components_ms);
    return 0;
}

// `--aggregate SEED` aggregates the graph of the final result's pattern (what --colour would colour; it
// must be square; both directions of every stored entry count) on the device (pem_tiled_aggregate): the MIS(2) aggregation in the
// order of the priorities SEED hashes.  One line reports aggregates, rounds and the time; --out then writes the aggregate ids
// (Matrix-Market `array integer general`, 1-based) instead of the matrix.  The CSV row describes the product.
static int aggregate_stage(const Options &o, pem_ctx *ctx, Result *r)
{
    Operand src;
    CHECK(src.open(ctx, *r));
    const pem_tiled_info &si = src.info;
    CHECK(pem_tiled_get_info(src.t, &src.info));
    if (si.rows != si.cols) {
        printf("--aggregate: %s is %d x %d; an aggregation needs a square matrix. Exiting.\n", r->last_name, si.rows, si.cols);
        return 1;
    }
    const size_t n = (size_t)si.rows;
    DevBuf da;
    if (!da.alloc(n, 4)) {
        fprintf(stderr, "pemspgemm: --aggregate: device allocation of %zu aggregate ids failed\n", n);
        return 2;
    }
    CHECK(pem_ctx_synchronize(ctx));
    int64_t naggregates = 0;
    int32_t rounds = 0;
    auto c0 = Clock::now();
    CHECK(pem_tiled_aggregate(ctx, src.t, 0, o.aggregate_seed, nullptr, (int32_t *)da.p, nullptr, &naggregates, &rounds));
    const double aggregate_ms = ms_since(c0);
    std::vector<int32_t> agg(n);
    if (n && hipMemcpy(agg.data(), da.p, 4 * n, hipMemcpyDeviceToHost) != hipSuccess) return 2;
    r->aggregates.resize(n);
    for (size_t v = 0; v < n; ++v) r->aggregates[v] = (double)(agg[v] + 1);
    printf("aggregate: seed %s of %s: %lld aggregates in %d rounds, %zu vertices, %.3fms\n", o.aggregate_spec, r->last_name,
           (long long)naggregates, rounds, n, aggregate_ms);
    return 0;
}

// `--spmm X.mtx` computes Y = R (+).(x) X on the device (pem_tiled_spmm), R the final result (C, the
// sum of --add, or what --select kept) and X a Matrix-Market `array real general` file of R.cols rows (read as float with
// --fp32); --out then writes Y (an array, R.rows x k) instead of the matrix.  The CSV row describes the product.
static int spmm_stage(const Options &o, pem_ctx *ctx, Result *r)
{
    Operand src;
    CHECK(src.open(ctx, *r));
    CHECK(pem_tiled_get_info(src.t, &src.info));
    if (o.spmm_rows != src.info.cols) {
        printf("--spmm %s: X has %lld rows; the result has %d columns. Exiting.\n", o.spmm_path, (long long)o.spmm_rows, src.info.cols);
        return 1;
    }
    const int64_t k = o.spmm_k, ld = k > 1 ? k : 1;
    r->spmm_ny = src.info.rows;
    const size_t nyv = (size_t)r->spmm_ny * (size_t)ld;
    DevBuf dx, dy;
    if (!dx.upload(o.spmm_x, (size_t)o.spmm_rows * (size_t)ld, o.fp32) || !dy.alloc(nyv, o.fp32 ? 4 : 8)) {
        fprintf(stderr, "pemspgemm: --spmm: device allocation failed\n");
        return 2;
    }
    CHECK(pem_ctx_synchronize(ctx));
    auto m0 = Clock::now();
    CHECK(o.fp32 ? pem_tiled_spmm_f32(ctx, src.t, o.semiring, 0, k, (const float *)dx.p, ld, (float *)dy.p, ld, 0)
                 : pem_tiled_spmm(ctx, src.t, o.semiring, 0, k, (const double *)dx.p, ld, (double *)dy.p, ld, 0));
    CHECK(pem_ctx_synchronize(ctx));
    const double spmm_ms = ms_since(m0);
    if (!dy.download(&r->spmm_y, nyv, o.fp32)) return 2;
    printf("spmm: Y = %s (%s) X: spmm %.3fms, k %lld, %lld x %lld values, host sum %.17g\n", r->last_name, semiring_names[o.semiring], spmm_ms,
           (long long)k, (long long)r->spmm_ny, (long long)k, sum_of(r->spmm_y));
    return 0;
}

// `--sddmm X.mtx [--sddmm-y Y.mtx]`: the final result R (C, the sum of --add, or what --select kept)
// gets the values of pattern(R) o (X Y^T) under the semiring, on the device (pem_tiled_sddmm); X and Y are Matrix-Market `array
// real general` files of R.rows and R.cols rows and the same k columns (read as float with --fp32), Y defaults to X.  Its CSR
// export serves --out and the sorted COO files.  The CSV row describes the product.
static int sddmm_stage(const Options &o, pem_ctx *ctx, Result *r)
{
    Operand src;
    CHECK(src.open(ctx, *r));
    const pem_tiled_info &si = src.info;
    CHECK(pem_tiled_get_info(src.t, &src.info));
    if (o.sddmm_xrows != si.rows) {
        printf("--sddmm %s: X has %lld rows; the result has %d rows. Exiting.\n", o.sddmm_path, (long long)o.sddmm_xrows, si.rows);
        return 1;
    }
    if (o.sddmm_yrows != si.cols) {
        printf("--sddmm%s %s: Y has %lld rows; the result has %d columns. Exiting.\n", o.sddmm_y_path ? "-y" : "",
               o.sddmm_y_path ? o.sddmm_y_path : o.sddmm_path, (long long)o.sddmm_yrows, si.cols);
        return 1;
    }
    const int64_t k = o.sddmm_k, ld = k > 1 ? k : 1;
    DevBuf dx, dy_own;
    if (!dx.upload(o.sddmm_x, (size_t)o.sddmm_xrows * (size_t)ld, o.fp32) ||
        (o.sddmm_y_path && !dy_own.upload(o.sddmm_y, (size_t)o.sddmm_yrows * (size_t)ld, o.fp32))) {
        fprintf(stderr, "pemspgemm: --sddmm: device allocation failed\n");
        return 2;
    }
    const void *dy = o.sddmm_y_path ? dy_own.p : dx.p;   // Y = X: the same pointer
    CHECK(pem_ctx_synchronize(ctx));
    auto m0 = Clock::now();
    CHECK(o.fp32 ? pem_tiled_sddmm_f32(ctx, src.t, o.semiring, k, (const float *)dx.p, ld, (const float *)dy, ld, out(ctx, r->sd))
                 : pem_tiled_sddmm(ctx, src.t, o.semiring, k, (const double *)dx.p, ld, (const double *)dy, ld, out(ctx, r->sd)));
    const double sd_ms = ms_since(m0);
    CHECK(export_csr(ctx, r->sd.get(), o.fp32, &r->sd_csr));
    printf("sddmm: R = pattern(%s) o (X %s^T) (%s): sddmm %.3fms, k %lld, nnz %lld, host sum %.17g\n", r->last_name, o.sddmm_y_path ? "Y" : "X",
           semiring_names[o.semiring], sd_ms, (long long)k, (long long)r->sd_csr.nnz(), sum_of(r->sd_csr.v));
    return 0;
}

// `--sampled S.mtx [--sampled-bt]` takes the place of the plan product: R = pattern(S) o (A*B) under the
// semiring by dot products on the device (pem_tiled_sampled_mxm), A*B^T from B's rows with --sampled-bt; --out gets R.
// `--triangles` prints the triangle count of A's pattern (symmetric, as the count assumes): with L = A's strict lower triangle,
// the sum of L o (L*L^T) under plus_pair.  No plan is made and no later stage runs.
static int sampled_stage(const Options &o, pem_ctx *ctx, const Operands &in)
{
    const auto t0 = Clock::now();
    Tiled L, R;
    Csr c;
    if (o.triangles) {
        CHECK(pem_tiled_select(ctx, in.A.get(), PEM_SELECT_TRIL, -1.0, out(ctx, L)));
        CHECK(pem_tiled_sampled_mxm(ctx, L.get(), L.get(), L.get(), 1, PEM_SEMIRING_PLUS_PAIR, out(ctx, R)));
        const double ms = ms_since(t0);
        CHECK(export_csr(ctx, R.get(), o.fp32, &c));
        long long n = 0;
        for (double v : c.v) n += (long long)v;
        printf("triangles: %lld (L o (L*L^T) under plus_pair, L = tril(A, -1) with %lld entries: %.3fms)\n", n, (long long)c.nnz(), ms);
        return 0;
    }
    CHECK(pem_tiled_sampled_mxm(ctx, in.Sp.get(), in.A.get(), in.B, o.sampled_bt ? 1 : 0, o.semiring, out(ctx, R)));
    const double ms = ms_since(t0);
    CHECK(export_csr(ctx, R.get(), o.fp32, &c));
    const char *const bt = o.aat || o.sampled_bt ? "^T" : "";
    printf("sampled: R = pattern(S) o (A*B%s) (%s): sampled_mxm %.3fms, nnz %lld, host sum %.17g\n", bt, semiring_names[o.semiring], ms,
           (long long)c.nnz(), sum_of(c.v));
    if (o.out_path)
        return write_mtx(o.out_path, c.rows, c.cols, c, std::string("R = pattern(S) o (A*B") + bt + ") (" + semiring_names[o.semiring] + ") by pemspgemm (pem-spgemm_amd)", "R");
    return 0;
}

// The sorted COO files of the 2nd argument: the sampled product's, the stacked matrix's, the Kronecker product's or the assigned matrix's entries when
// there is one (their CSR export is the sorted (row, column) order), else the plan's C as the reference writes it.
static int save_stage(const Options &o, pem_ctx *ctx, Result *r)
{
    if (!o.save) {
        printf("Not saving results. Exiting.\n");   // spgemm.cu:1487
    } else if (r->sd) {
        r->rc = save_result_files(r->sd_csr.rp, r->sd_csr.ci, r->sd_csr.v);
    } else if (r->stk || r->krn || r->asg) {
        Csr c;
        CHECK(export_csr(ctx, r->stk ? r->stk.get() : r->krn ? r->krn.get() : r->asg.get(), o.fp32, &c));
        r->rc = save_result_files(c.rp, c.ci, c.v);
    } else {
        Csr c;   // as COO
        CHECK(export_coo(ctx, r->plan.get(), r->ci, o.fp32, &c));
        pem_timings t;
        CHECK(pem_get_timings(ctx, &t));
        printf("sanitize_C took %.2fms\n", t.export_ms);
        r->rc = save_coo_files(c.nnz(), c.rp.data(), c.ci.data(), c.v.data());
    }
    return 0;
}

// `--out <file>`: x of --trsv, else x of --solve, else the levels of --bfs, else the parents of --bfs-parents, else the colours of --colour, else the labels of --components, else the aggregate ids of --aggregate, else the indices of --argreduce, else Y of --spmm, else the vector of --reduce (Matrix-Market dense arrays), else the
// matrix: the sampled product of --sddmm, the final result when it is a tiling (its CSR export), or the plan's C (CSR export:
// rows ascending, columns ascending).  The comment line says how the matrix came about.
static int out_stage(const Options &o, pem_ctx *ctx, const Operands &in, Result *r)
{
    const char *const semiring = semiring_names[o.semiring];
    std::string how;   // of a matrix: what --select, --extract-* and --assign-into did to it
    if (r->app) how += std::string(", apply ") + o.apply_spec;
    if (r->scl)
        how += std::string(", scale ") + binop_names[o.scale_op] + (o.scale_paths[0] ? std::string(" rows ") + o.scale_paths[0] : std::string()) +
               (o.scale_paths[1] ? std::string(" columns ") + o.scale_paths[1] : std::string());
    if (r->sel) how += std::string(r->sd ? ", C after select " : ", select ") + o.select_spec;
    if (r->top) how += std::string(", topk ") + o.topk_spec;
    if (r->ext)
        how += std::string(", extract ") + (o.extract_paths[0] ? std::string("rows ") + o.extract_paths[0] : std::string()) +
               (o.extract_paths[0] && o.extract_paths[1] ? ", " : "") + (o.extract_paths[1] ? std::string("columns ") + o.extract_paths[1] : std::string());
    if (r->asg)
        how += std::string(", assigned into ") + o.assign_into + (o.assign_paths[0] ? std::string(" rows ") + o.assign_paths[0] : std::string()) +
               (o.assign_paths[1] ? std::string(" columns ") + o.assign_paths[1] : std::string()) +
               (o.assign_accum == PEM_ACCUM_NONE ? std::string() : std::string(" accum ") + binop_names[o.assign_accum]);
    if (r->krn) how += std::string(", kron ") + binop_names[o.kron_op] + " with " + o.kron_path;
    if (r->stk) how += std::string(o.stack_paths[1] ? ", vstack with " : ", hstack with ") + o.stack_paths[o.stack_paths[1] ? 1 : 0];
    if (r->ilu) how += ", its ILU(0) factor (L strictly below the diagonal, unit diagonal not stored; U on and above)";
    how += " by pemspgemm (pem-spgemm_amd)";
    int rc = 0;
    if (o.trsv_uplo >= 0) {
        rc = write_mm_array(o.out_path, "real", std::string("x of T x = b, T the ") + o.trsv_spec + " triangle of C = A*B" + (o.rhs_path ? std::string(", b ") + o.rhs_path : std::string(", b all ones")),
                            (int64_t)r->trsv_x.size(), 1, r->trsv_x, 1, o.fp32, "the ", "solution");
    } else if (o.solve_method >= 0) {
        rc = write_mm_array(o.out_path, "real", std::string("x of C x = b by ") + o.solve_spec + ", C = A*B, b " + o.rhs_path, (int64_t)r->solve_x.size(), 1,
                            r->solve_x, 1, o.fp32, "the ", "solution");
    } else if (o.bfs_spec) {
        rc = write_mm_array(o.out_path, "integer", "bfs levels from " + std::to_string(o.bfs_src), (int64_t)r->bfs_levels.size(), 1, r->bfs_levels, 1,
                            false, "the ", "levels");
    } else if (o.bfs_parents_spec) {
        rc = write_mm_array(o.out_path, "integer", "bfs parents from " + std::to_string(o.bfs_parents_src) + " (1-based, 0: unreachable)",
                            (int64_t)r->bfs_parents.size(), 1, r->bfs_parents, 1, false, "the ", "parents");
    } else if (o.colour_flag()) {
        rc = write_mm_array(o.out_path, "integer", std::string("greedy colours of the pattern of C = A*B, ") + (o.colour_natural ? "natural order" : std::string("seed ") + o.colour_spec) + " (1-based)",
                            (int64_t)r->colours.size(), 1, r->colours, 1, false, "the ", "colours");
    } else if (o.components) {
        rc = write_mm_array(o.out_path, "integer", "connected components of the pattern of C = A*B: the smallest vertex of every vertex's component (1-based)",
                            (int64_t)r->labels.size(), 1, r->labels, 1, false, "the ", "labels");
    } else if (o.aggregate_spec) {
        rc = write_mm_array(o.out_path, "integer", std::string("MIS(2) aggregates of the pattern of C = A*B, seed ") + o.aggregate_spec + " (1-based)",
                            (int64_t)r->aggregates.size(), 1, r->aggregates, 1, false, "the ", "aggregates");
    } else if (o.argreduce_dim >= 0) {
        rc = write_mm_array(o.out_path, "integer", std::string("argreduce ") + o.argreduce_spec + " of C = A*B (1-based, 0: no entry)",
                            (int64_t)r->arg_idx.size(), 1, r->arg_idx, 1, false, "the ", "indices");
    } else if (o.spmm_path) {
        rc = write_mm_array(o.out_path, "real", std::string("Y = R X (") + semiring + ")", r->spmm_ny, o.spmm_k, r->spmm_y, o.spmm_k > 1 ? o.spmm_k : 1,
                            o.fp32, "", "Y");
    } else if (o.reduce_dim >= 0) {
        rc = write_mm_array(o.out_path, "real", std::string("reduce ") + o.reduce_spec + " of C = A*B (" + semiring + ")", (int64_t)r->red.size(), 1,
                            r->red, 1, o.fp32, "the ", "vector");
    } else if (r->sd) {
        pem_tiled_info si;
        CHECK(pem_tiled_get_info(r->sd.get(), &si));
        rc = write_mtx(o.out_path, si.rows, si.cols, r->sd_csr, std::string("R = pattern(C) o (X Y^T) (") + semiring + ")" + how, "R");
    } else if (r->last) {
        Csr c;
        CHECK(export_csr(ctx, r->last, o.fp32, &c));
        rc = write_mtx(o.out_path, c.rows, c.cols, c, std::string(r->sum ? "C = alpha*A*B + beta*D (" : "C = A*B (") + semiring + ")" + how, "C");
    } else {
        Csr c;
        CHECK(export_csr(ctx, r->plan.get(), r->ci, o.fp32, &c));
        const std::string over = o.semiring == PEM_SEMIRING_PLUS_TIMES ? std::string() : std::string(" over the ") + semiring + " semiring";
        rc = write_mtx(o.out_path, in.ia.rows, in.ib.cols, c, "C = A*B" + over + how, "C");
    }
    if (rc) r->rc = rc;
    return 0;
}

// The table of contents: options, then either the --gpus path or the context, the operands and the stages in order.  Everything
// made on the device is owned by Operands and Result, which are declared after the context and so released before it.
int main(int argc, char *argv[])
{
    Options o;
    parse_args(argc, argv, &o);
    if (int rc = validate(&o)) return rc;
    if (o.ngpu > 0) return run_gpus(o);

    Ctx ctx_own;   // device + memory set-up precede the conversion clock, as in the reference (spgemm.cu:730-758)
    CHECK(pem_ctx_create(env_int("PEM_DEVICE", 0), out(nullptr, ctx_own)));
    pem_ctx *const ctx = ctx_own.get();
    Operands in;
    Result r;
    int rc = build_operands(o, ctx, &in);
    if (!rc && (o.sampled_path || o.triangles)) {
        if ((rc = sampled_stage(o, ctx, in))) return rc;
        printf("CLEANING UP RESOURCES\n\n");
        return 0;
    }
    if (!rc) rc = power_prologue(o, ctx, &in, &r);
    if (!rc) rc = timed_product(o, ctx, in, &r);
    if (!rc && in.Dt) rc = add_stage(o, ctx, in, &r);
    if (!rc && o.apply_op >= 0) rc = apply_stage(o, ctx, &r);
    if (!rc && (o.scale_paths[0] || o.scale_paths[1])) rc = scale_stage(o, ctx, &r);
    if (!rc && o.select_op >= 0) rc = select_stage(o, ctx, &r);
    if (!rc && o.topk_order >= 0) rc = topk_stage(o, ctx, &r);
    if (!rc && (o.extract_paths[0] || o.extract_paths[1])) rc = extract_stage(o, ctx, &r);
    if (!rc && in.Into) rc = assign_stage(o, ctx, in, &r);
    if (!rc && in.Kt) rc = kron_stage(o, ctx, in, &r);
    if (!rc && in.St) rc = stack_stage(o, ctx, in, &r);
    if (!rc && o.ilu0) rc = ilu0_stage(o, ctx, &r);
    if (!rc && o.reduce_dim >= 0) rc = reduce_stage(o, ctx, &r);
    if (!rc && o.trsv_uplo >= 0) rc = trsv_stage(o, ctx, &r);
    if (!rc && o.solve_method >= 0) rc = solve_stage(o, ctx, &r);
    if (!rc && o.bfs_spec) rc = bfs_stage(o, ctx, &r);
    if (!rc && o.argreduce_dim >= 0) rc = argreduce_stage(o, ctx, &r);
    if (!rc && o.bfs_parents_spec) rc = bfs_parents_stage(o, ctx, &r);
    if (!rc && o.colour_flag()) rc = colour_stage(o, ctx, &r);
    if (!rc && o.components) rc = components_stage(o, ctx, &r);
    if (!rc && o.aggregate_spec) rc = aggregate_stage(o, ctx, &r);
    if (!rc && o.spmm_path) rc = spmm_stage(o, ctx, &r);
    if (!rc && o.sddmm_path) rc = sddmm_stage(o, ctx, &r);
    if (!rc) rc = save_stage(o, ctx, &r);
    if (!rc && o.out_path) rc = out_stage(o, ctx, in, &r);
    if (rc) return rc;   // a refusal or a failed call: the message has been printed
    printf("CLEANING UP RESOURCES\n\n");
    return r.rc;
}
