// pemspgemm -- command-line front end with the reference's surface (spgemm.cu:720-1568):
//     pemspgemm <matrix.mtx> [0|1] [any third argument => C = A*A^T]
// reads one Matrix-Market file, forms C = A*A (or A*A^T), times WARMUP + REPEAT passes of
// step1+step2+step3, prints the reference's report, appends the reference's 14 CSV columns
// to ./pemspgemm_benchmark_result.csv and, when the 2nd argument is non-zero, writes the
// sorted COO result to /tmp/SPGEMM_RESULT_{NNZ,ROWS,COLS,VALS}.txt.
// Host C++ over the C ABI of libpemspgemm_hip.so; no HIP calls in this file.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cctype>
#include <cmath>
#include <condition_variable>
#include <mutex>
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

// the input: a Matrix-Market file (spgemm.cu:43-110), or "standin:NAME" for the seeded generator (--standin)
static double g_standin_scale = 1.0;
static int read_input(const char *path, pem_coo *out)
{
    if (!strncmp(path, "standin:", 8)) {
        const int rc = pem_standin_generate(path + 8, g_standin_scale, out);
        if (rc != 0) fprintf(stderr, "pemspgemm: --standin %s (scale %g): no such stand-in (have: %s) or bad scale\n", path + 8, g_standin_scale, pem_standin_names());
        return rc;
    }
    const int rc = pem_mm_read(path, 0, out);
    if (rc != 0) fprintf(stderr, "pemspgemm: %s\n", pem_host_last_error());
    return rc;
}

// --spmm: X as a Matrix-Market `array real general` file (values column by column), returned row-major (x[j * k + c]).  Returns an
// empty string on success, else what is wrong.  (pem_mm_read reads coordinate files only.)
static std::string read_dense_array(const char *path, int64_t *rows, int64_t *k, std::vector<double> *x)
{
    FILE *f = fopen(path, "r");
    if (!f) return "cannot open the file";
    char line[4096];
    std::string err;
    if (!fgets(line, sizeof line, f)) err = "empty file";
    char banner[64] = "", object[64] = "", format[64] = "", field[64] = "", symmetry[64] = "";
    if (err.empty() && sscanf(line, "%63s %63s %63s %63s %63s", banner, object, format, field, symmetry) != 5) err = "no Matrix-Market header";
    auto lower = [](char *t) { for (; *t; ++t) *t = (char)tolower((unsigned char)*t); };
    lower(banner), lower(object), lower(format), lower(field), lower(symmetry);
    if (err.empty() && (strcmp(banner, "%%matrixmarket") || strcmp(object, "matrix"))) err = "no Matrix-Market header";
    if (err.empty() && strcmp(format, "array")) err = std::string("a ") + format + " file, not an array (dense) file";
    if (err.empty() && strcmp(field, "real")) err = std::string("a ") + field + " file, not a real one";
    if (err.empty() && strcmp(symmetry, "general")) err = std::string("a ") + symmetry + " array, not a general one";
    long long m = -1, n = -1;
    while (err.empty()) {
        if (!fgets(line, sizeof line, f)) {
            err = "no size line";
            break;
        }
        if (line[0] == '%') continue;
        if (sscanf(line, "%lld %lld", &m, &n) != 2 || m < 0 || n < 0) err = "bad size line";
        break;
    }
    if (err.empty()) {
        x->assign((size_t)m * (size_t)n, 0.0);
        for (long long c = 0; c < n && err.empty(); ++c)
            for (long long j = 0; j < m; ++j) {
                double v;
                if (fscanf(f, "%lf", &v) != 1) {
                    err = "fewer values than rows x cols";
                    break;
                }
                (*x)[(size_t)j * (size_t)n + (size_t)c] = v;
            }
    }
    fclose(f);
    *rows = m, *k = n;
    return err;
}

// An index list of --extract-rows / --extract-cols: a Matrix-Market `array` file of one column, `integer` or `real` with integral
// values, holding 1-based indices like a coordinate file; idx receives them 0-based.  "" or what is wrong with the file.
static std::string read_index_array(const char *path, std::vector<int32_t> *idx)
{
    FILE *f = fopen(path, "r");
    if (!f) return "cannot open the file";
    char line[4096];
    std::string err;
    if (!fgets(line, sizeof line, f)) err = "empty file";
    char banner[64] = "", object[64] = "", format[64] = "", field[64] = "", symmetry[64] = "";
    if (err.empty() && sscanf(line, "%63s %63s %63s %63s %63s", banner, object, format, field, symmetry) != 5) err = "no Matrix-Market header";
    auto lower = [](char *t) { for (; *t; ++t) *t = (char)tolower((unsigned char)*t); };
    lower(banner), lower(object), lower(format), lower(field), lower(symmetry);
    if (err.empty() && (strcmp(banner, "%%matrixmarket") || strcmp(object, "matrix"))) err = "no Matrix-Market header";
    if (err.empty() && strcmp(format, "array")) err = std::string("a ") + format + " file, not an array (dense) file";
    if (err.empty() && strcmp(field, "integer") && strcmp(field, "real")) err = std::string("a ") + field + " file, not an integer or real one";
    if (err.empty() && strcmp(symmetry, "general")) err = std::string("a ") + symmetry + " array, not a general one";
    long long m = -1, n = -1;
    while (err.empty()) {
        if (!fgets(line, sizeof line, f)) {
            err = "no size line";
            break;
        }
        if (line[0] == '%') continue;
        if (sscanf(line, "%lld %lld", &m, &n) != 2 || m < 0 || n < 0) err = "bad size line";
        break;
    }
    if (err.empty() && n != 1) err = "an array of " + std::to_string(n) + " columns, not of one";
    if (err.empty() && (m < 1 || m > 2147483647ll)) err = "a list of " + std::to_string(m) + " indices, not of 1 .. 2^31 - 1";
    if (err.empty()) {
        idx->assign((size_t)m, 0);
        for (long long j = 0; j < m; ++j) {
            double v;
            if (fscanf(f, "%lf", &v) != 1) {
                err = "fewer values than the size line says";
                break;
            }
            if (!(std::floor(v) == v)) {
                err = "index " + std::to_string(j + 1) + " is not an integer";
                break;
            }
            if (!(v >= 1.0 && v <= 2147483647.0)) {
                err = "index " + std::to_string(j + 1) + " is out of range (indices are 1-based)";
                break;
            }
            (*idx)[(size_t)j] = (int32_t)((long long)v - 1);
        }
    }
    fclose(f);
    return err;
}

int main(int argc, char *argv[])
{
    // Beyond the reference: `--B <file.mtx>` multiplies by a second matrix instead of A itself,
    // `--out <file.mtx>` writes C as a Matrix-Market file.  They are stripped before the reference's own grammar.
    // `--cache <dir>` keeps each tiling as <dir>/<stem>.<A|AT>.pemtile and, while the .mtx is unchanged
    // (size + mtime), loads it instead of parsing and converting.
    // `--fp32` computes in float: the values are rounded once at conversion, step 3 runs one fmaf per product.
    // `--gpus N`: N tile-row blocks of A on N devices, C gathered to device 0 over RCCL (see run_multi); the blocks are
    // re-cut from measured pass times first (`--no-tune-split` keeps the product-balanced cut), and the product is also run as
    // `--chunks K` chunks per rank with the gather overlapped (default: K from C's size; 0: off).
    // `--mask <M.mtx>` computes the masked product C<M> = A*B: only the entries at M's stored positions (pem_cplan_create_masked);
    // with `--mask-complement` only those where M stores nothing.  M has C's shape; the flop count stays the unmasked product's.
    // `--semiring NAME`: step 3 reduces under plus_times (default), min_plus, max_plus, max_times,
    // plus_pair or lor_land; C's structure, the flop count (the tile product's) and the CSV columns do not change.
    // `--power K` computes A^K = (...(A*A)*A...)*A as K-1 products, every C turned into the next left
    // operand on the device; with --semiring every product uses it.  The report and the CSV row describe the last product.
    // `--add D.mtx [--alpha x] [--beta y]` computes C = alpha*(A*B) (+) beta*D on the device: the product's
    // C becomes a tiling (pem_tiled_from_cplan) and is combined with D over the union of their patterns (pem_tiled_ewise), (+) being
    // the semiring's additive op; --out then writes that sum.  D has C's shape and is read with --fp32 like A.
    // `--select OP[:THUNK]` keeps the entries of the final result (C, or the sum of --add) that satisfy
    // OP, one of tril triu diag offdiag row_le row_gt col_le col_gt (THUNK an integer k) or value_eq value_ne value_lt value_le
    // value_gt value_ge abs_gt (THUNK a value); THUNK defaults to 0.  The result becomes a tiling (pem_tiled_from_cplan, or the
    // ewise sum) and is filtered on the device (pem_tiled_select); --out then writes what is kept.  The CSV row describes the product.
    // `--extract-rows I.mtx` / `--extract-cols J.mtx`, either or both: the final result R (C, the sum of
    // --add, or what --select kept) becomes R(I, J) on the device (pem_tiled_extract).  Each file is a Matrix-Market `array` file of
    // one column holding 1-based indices (`integer`, or `real` with integral values), in any order, repeats allowed.  --reduce,
    // --spmm, --sddmm and --out then see the extracted tiling.  The CSV row describes the product.
    // `--assign-into D.mtx [--assign-rows I.mtx] [--assign-cols J.mtx] [--assign-accum OP]`: after the
    // product and any --add / --select / --extract-*, the final result R is written into D at (I, J) on the device (pem_tiled_assign):
    // D(I, J) = R, or D(I, J) = OP(D(I, J), R) with OP one of plus times min max lor land.  The lists are files like --extract-rows'
    // (1-based, any order, no repeats; absent = all); R must be |I| x |J|.  D is read with --fp32 like A.  --reduce, --spmm, --sddmm,
    // --out and the sorted COO files then see that tiling.  The CSV row describes the product.
    // `--reduce rows|cols[:OP]` folds every row or column of the final result (C, the sum of --add, or
    // what --select kept) on the device (pem_tiled_reduce); OP is one of plus times min max lor land and defaults to the semiring's
    // additive op.  --out then writes the vector (Matrix-Market array) instead of the matrix.  The CSV row describes the product.
    // `--bfs SRC` runs a breadth-first search from the 1-based vertex SRC over the pattern of the final
    // result (what --reduce would fold; it must be square) on the device (pem_tiled_bfs): a stored entry (i, j) is an edge i -> j.
    // One line reports depth, reached and the time; --out then writes the levels (Matrix-Market `array integer general`, -1 for
    // unreachable) instead of the matrix.  The CSV row describes the product.
    // `--spmm X.mtx` computes Y = R (+).(x) X on the device (pem_tiled_spmm), R the final result (C, the
    // sum of --add, or what --select kept) and X a Matrix-Market `array real general` file of R.cols rows (read as float with
    // --fp32); --out then writes Y (an array, R.rows x k) instead of the matrix.  The CSV row describes the product.
    // `--sddmm X.mtx [--sddmm-y Y.mtx]`: the final result R (C, the sum of --add, or what --select kept)
    // gets the values of pattern(R) o (X Y^T) under the semiring, on the device (pem_tiled_sddmm); X and Y are Matrix-Market `array
    // real general` files of R.rows and R.cols rows and the same k columns (read as float with --fp32), Y defaults to X.  --out and
    // the sorted COO files then receive that tiling.  The CSV row describes the product.
    // `--standin NAME [--scale S]`: the seeded C++ stand-in generator takes the place of the file (no SuiteSparse
    // file exists offline); NAME then stands where the path stood, and the remaining positional arguments keep their meaning.
    const char *b_path = nullptr, *out_path = nullptr, *cache_dir = nullptr, *standin = nullptr, *mask_path = nullptr;
    bool mask_complement = false;
    const char *semiring_name = nullptr;
    int power = 0;   // --power K: A^K as K-1 chained products (0: off)
    const char *add_path = nullptr;   // --add D.mtx: C = alpha*(A*B) (+) beta*D
    double add_alpha = 1.0, add_beta = 1.0;
    const char *select_spec = nullptr;   // --select OP[:THUNK]
    const char *extract_paths[2] = {nullptr, nullptr};   // --extract-rows I.mtx, --extract-cols J.mtx
    const char *assign_into = nullptr, *assign_accum_name = nullptr;   // --assign-into D.mtx, --assign-accum OP
    const char *assign_paths[2] = {nullptr, nullptr};                  // --assign-rows I.mtx, --assign-cols J.mtx
    const char *reduce_spec = nullptr;   // --reduce rows|cols[:OP]
    const char *bfs_spec = nullptr;      // --bfs SRC
    const char *spmm_path = nullptr;     // --spmm X.mtx
    const char *sddmm_path = nullptr, *sddmm_y_path = nullptr;   // --sddmm X.mtx [--sddmm-y Y.mtx]
    static std::string standin_path;
    static std::vector<char *> argv_store;
    bool fp32 = false, tune_split = true;
    int ngpu = 0;   // 0: the reference's single-device path
    int nchunks = -1;   // --gpus: chunks per rank of the overlapped pass (-1: from C's size, 0: off)
    {
        int w = 1;
        for (int r = 1; r < argc; ++r) {
            if (!strcmp(argv[r], "--B") && r + 1 < argc) b_path = argv[++r];
            else if (!strcmp(argv[r], "--standin") && r + 1 < argc) standin = argv[++r];
            else if (!strcmp(argv[r], "--scale") && r + 1 < argc) g_standin_scale = atof(argv[++r]);
            else if (!strcmp(argv[r], "--gpus") && r + 1 < argc) ngpu = atoi(argv[++r]);
            else if (!strcmp(argv[r], "--out") && r + 1 < argc) out_path = argv[++r];
            else if (!strcmp(argv[r], "--cache") && r + 1 < argc) cache_dir = argv[++r];
            else if (!strcmp(argv[r], "--fp32")) fp32 = true;
            else if (!strcmp(argv[r], "--mask") && r + 1 < argc) mask_path = argv[++r];
            else if (!strcmp(argv[r], "--mask-complement")) mask_complement = true;
            else if (!strcmp(argv[r], "--semiring") && r + 1 < argc) semiring_name = argv[++r];
            else if (!strcmp(argv[r], "--power") && r + 1 < argc) power = atoi(argv[++r]);
            else if (!strcmp(argv[r], "--add") && r + 1 < argc) add_path = argv[++r];
            else if (!strcmp(argv[r], "--alpha") && r + 1 < argc) add_alpha = atof(argv[++r]);
            else if (!strcmp(argv[r], "--beta") && r + 1 < argc) add_beta = atof(argv[++r]);
            else if (!strcmp(argv[r], "--select") && r + 1 < argc) select_spec = argv[++r];
            else if (!strcmp(argv[r], "--extract-rows") && r + 1 < argc) extract_paths[0] = argv[++r];
            else if (!strcmp(argv[r], "--extract-cols") && r + 1 < argc) extract_paths[1] = argv[++r];
            else if (!strcmp(argv[r], "--assign-into") && r + 1 < argc) assign_into = argv[++r];
            else if (!strcmp(argv[r], "--assign-rows") && r + 1 < argc) assign_paths[0] = argv[++r];
            else if (!strcmp(argv[r], "--assign-cols") && r + 1 < argc) assign_paths[1] = argv[++r];
            else if (!strcmp(argv[r], "--assign-accum") && r + 1 < argc) assign_accum_name = argv[++r];
            else if (!strcmp(argv[r], "--reduce") && r + 1 < argc) reduce_spec = argv[++r];
            else if (!strcmp(argv[r], "--bfs") && r + 1 < argc) bfs_spec = argv[++r];
            else if (!strcmp(argv[r], "--spmm") && r + 1 < argc) spmm_path = argv[++r];
            else if (!strcmp(argv[r], "--sddmm") && r + 1 < argc) sddmm_path = argv[++r];
            else if (!strcmp(argv[r], "--sddmm-y") && r + 1 < argc) sddmm_y_path = argv[++r];
            else if (!strcmp(argv[r], "--no-tune-split")) tune_split = false;
            else if (!strcmp(argv[r], "--chunks") && r + 1 < argc) nchunks = atoi(argv[++r]);
            else argv[w++] = argv[r];
        }
        argc = w;
        if (standin) {
            standin_path = std::string("standin:") + standin;
            argv_store.assign(argv, argv + argc);
            argv_store.insert(argv_store.begin() + 1, const_cast<char *>(standin_path.c_str()));
            argv = argv_store.data();
            ++argc;
        }
    }
    if (argc <= 1 || argc > 4) {   // spgemm.cu:722-725
        printf("Provide a matrix market file path. Exiting.\n");
        return 1;
    }
    const int WARMUP = env_int("PEM_WARMUP", 1);    // spgemm.cu:712-714
    const int REPEAT = env_int("PEM_REPEAT", 10);   // reference Makefile:34 (-DREPEAT=10)
    const bool fastest = env_int("PEM_FASTEST", 0) != 0;   // spgemm.cu:1359-1363
    const bool save = argc >= 3 && atoi(argv[2]) != 0;     // spgemm.cu:1485 (the reference dereferences argv[2] unconditionally)
    const bool aat = argc == 4;                            // spgemm.cu:788: presence of a 3rd argument, value ignored

    if (mask_complement && !mask_path) {
        printf("--mask-complement needs --mask <M.mtx>. Exiting.\n");
        return 1;
    }
    static const char *const semiring_names[] = {"plus_times", "min_plus", "max_plus", "max_times", "plus_pair", "lor_land"};   // pem_semiring
    int semiring = PEM_SEMIRING_PLUS_TIMES;
    if (semiring_name) {
        semiring = -1;
        for (int i = 0; i < 6; ++i)
            if (!strcmp(semiring_name, semiring_names[i])) semiring = i;
        if (semiring < 0) {
            printf("--semiring %s: unknown semiring (plus_times, min_plus, max_plus, max_times, plus_pair, lor_land). Exiting.\n", semiring_name);
            return 1;
        }
    }
    if (ngpu > 0 && semiring != PEM_SEMIRING_PLUS_TIMES) {
        printf("--gpus does not combine with --semiring %s (the multi-GPU path multiplies under plus_times). Exiting.\n", semiring_names[semiring]);
        return 1;
    }
    if (power != 0) {
        const char *clash = power < 2 ? "K >= 2" : ngpu > 0 ? "--gpus" : mask_path ? "--mask" : b_path ? "--B" : aat ? "the A*A^T argument" : nullptr;
        if (clash) {
            if (power < 2)
                printf("--power %d: K must be at least 2. Exiting.\n", power);
            else
                printf("--power does not combine with %s (A^K multiplies A by itself on one device). Exiting.\n", clash);
            return 1;
        }
    }
    // --add: the semiring's additive op (pem_binop) combines alpha*C and beta*D
    static const int add_ops[] = {PEM_BINOP_PLUS, PEM_BINOP_MIN, PEM_BINOP_MAX, PEM_BINOP_MAX, PEM_BINOP_PLUS, PEM_BINOP_LOR};   // by pem_semiring
    static const char *const add_op_names[] = {"plus", "times", "min", "max", "lor", "land"};                                  // by pem_binop
    if (add_path) {
        const char *clash = ngpu > 0 ? "--gpus" : mask_path ? "--mask" : power ? "--power" : nullptr;
        if (clash) {
            printf("--add does not combine with %s. Exiting.\n", clash);
            return 1;
        }
        if ((add_alpha != 1.0 || add_beta != 1.0) && semiring != PEM_SEMIRING_PLUS_TIMES) {
            printf("--add: --alpha / --beta other than 1 need the plus_times semiring, not %s. Exiting.\n", semiring_names[semiring]);
            return 1;
        }
    } else if (add_alpha != 1.0 || add_beta != 1.0) {
        printf("--alpha / --beta need --add <D.mtx>. Exiting.\n");
        return 1;
    }
    // --select: the op by name (pem_select_op) and its thunk
    static const char *const select_names[] = {"tril",     "triu",     "diag",     "offdiag",  "row_le",   "row_gt",   "col_le", "col_gt",
                                               "value_eq", "value_ne", "value_lt", "value_le", "value_gt", "value_ge", "abs_gt"};
    int select_op = -1;
    double select_thunk = 0.0;
    if (select_spec) {
        const char *clash = ngpu > 0 ? "--gpus" : power ? "--power" : nullptr;
        if (clash) {
            printf("--select does not combine with %s. Exiting.\n", clash);
            return 1;
        }
        const char *colon = strchr(select_spec, ':');
        const std::string name = colon ? std::string(select_spec, (size_t)(colon - select_spec)) : std::string(select_spec);
        for (int i = 0; i < 15; ++i)
            if (name == select_names[i]) select_op = i;
        if (select_op < 0) {
            printf("--select %s: unknown op %s (tril, triu, diag, offdiag, row_le, row_gt, col_le, col_gt, value_eq, value_ne, value_lt, "
                   "value_le, value_gt, value_ge, abs_gt). Exiting.\n", select_spec, name.c_str());
            return 1;
        }
        if (colon) {
            char *end = nullptr;
            select_thunk = strtod(colon + 1, &end);
            if (end == colon + 1 || *end != '\0') {
                printf("--select %s: the thunk %s does not parse as a number. Exiting.\n", select_spec, colon + 1);
                return 1;
            }
        }
        if (select_op <= PEM_SELECT_COL_GT && !(std::floor(select_thunk) == select_thunk && std::fabs(select_thunk) <= 2147483648.0)) {
            printf("--select %s: the positional op %s needs an integral thunk k with |k| <= 2^31. Exiting.\n", select_spec, name.c_str());
            return 1;
        }
    }
    // --extract-rows / --extract-cols: the lists read up front, so that a bad file is refused before any work
    static const char *const extract_flags[2] = {"--extract-rows", "--extract-cols"};
    std::vector<int32_t> extract_idx[2];
    for (int q = 0; q < 2; ++q) {
        if (!extract_paths[q]) continue;
        const char *clash = ngpu > 0 ? "--gpus" : power ? "--power" : nullptr;
        if (clash) {
            printf("%s does not combine with %s. Exiting.\n", extract_flags[q], clash);
            return 1;
        }
        const std::string err = read_index_array(extract_paths[q], &extract_idx[q]);
        if (!err.empty()) {
            printf("%s %s: %s (want a Matrix-Market array file of one column of 1-based indices). Exiting.\n", extract_flags[q], extract_paths[q],
                   err.c_str());
            return 1;
        }
    }
    // --assign-into: the accum by name and the lists read up front, so that a bad option or file is refused before any work
    static const char *const assign_flags[2] = {"--assign-rows", "--assign-cols"};
    std::vector<int32_t> assign_idx[2];
    int assign_accum = PEM_ACCUM_NONE;
    if (!assign_into) {
        const char *lone = assign_paths[0] ? assign_flags[0] : assign_paths[1] ? assign_flags[1] : assign_accum_name ? "--assign-accum" : nullptr;
        if (lone) {
            printf("%s needs --assign-into <D.mtx>. Exiting.\n", lone);
            return 1;
        }
    } else {
        const char *clash = ngpu > 0 ? "--gpus" : power ? "--power" : nullptr;
        if (clash) {
            printf("--assign-into does not combine with %s. Exiting.\n", clash);
            return 1;
        }
        if (assign_accum_name) {
            for (int i = 0; i < 6; ++i)
                if (!strcmp(assign_accum_name, add_op_names[i])) assign_accum = i;
            if (assign_accum == PEM_ACCUM_NONE) {
                printf("--assign-accum %s: unknown op (plus, times, min, max, lor, land). Exiting.\n", assign_accum_name);
                return 1;
            }
        }
        for (int q = 0; q < 2; ++q) {
            if (!assign_paths[q]) continue;
            const std::string err = read_index_array(assign_paths[q], &assign_idx[q]);
            if (!err.empty()) {
                printf("%s %s: %s (want a Matrix-Market array file of one column of 1-based indices). Exiting.\n", assign_flags[q], assign_paths[q],
                       err.c_str());
                return 1;
            }
            std::vector<int32_t> sorted(assign_idx[q]);
            std::sort(sorted.begin(), sorted.end());
            const auto dup = std::adjacent_find(sorted.begin(), sorted.end());
            if (dup != sorted.end()) {
                printf("%s %s: index %d is repeated; assign is defined for lists without repeats only. Exiting.\n", assign_flags[q], assign_paths[q],
                       *dup + 1);
                return 1;
            }
        }
    }
    // --spmm: X read up front, so that a bad file is refused before any work
    int64_t spmm_rows = 0, spmm_k = 0;
    std::vector<double> spmm_x;
    if (spmm_path) {
        const char *clash = ngpu > 0 ? "--gpus" : power ? "--power" : reduce_spec ? "--reduce" : nullptr;
        if (clash) {
            printf("--spmm does not combine with %s. Exiting.\n", clash);
            return 1;
        }
        const std::string err = read_dense_array(spmm_path, &spmm_rows, &spmm_k, &spmm_x);
        if (!err.empty()) {
            printf("--spmm %s: %s (want a Matrix-Market array real general file). Exiting.\n", spmm_path, err.c_str());
            return 1;
        }
    }
    // --sddmm: X and Y read up front, so that a bad file is refused before any work
    int64_t sddmm_xrows = 0, sddmm_yrows = 0, sddmm_k = 0;
    std::vector<double> sddmm_x, sddmm_y;
    if (sddmm_y_path && !sddmm_path) {
        printf("--sddmm-y needs --sddmm <X.mtx>. Exiting.\n");
        return 1;
    }
    if (sddmm_path) {
        const char *clash = ngpu > 0 ? "--gpus" : power ? "--power" : reduce_spec ? "--reduce" : spmm_path ? "--spmm" : nullptr;
        if (clash) {
            printf("--sddmm does not combine with %s. Exiting.\n", clash);
            return 1;
        }
        std::string err = read_dense_array(sddmm_path, &sddmm_xrows, &sddmm_k, &sddmm_x);
        if (!err.empty()) {
            printf("--sddmm %s: %s (want a Matrix-Market array real general file). Exiting.\n", sddmm_path, err.c_str());
            return 1;
        }
        if (sddmm_y_path) {
            int64_t ky = 0;
            err = read_dense_array(sddmm_y_path, &sddmm_yrows, &ky, &sddmm_y);
            if (!err.empty()) {
                printf("--sddmm-y %s: %s (want a Matrix-Market array real general file). Exiting.\n", sddmm_y_path, err.c_str());
                return 1;
            }
            if (ky != sddmm_k) {
                printf("--sddmm-y %s: Y has %lld columns, X has %lld. Exiting.\n", sddmm_y_path, (long long)ky, (long long)sddmm_k);
                return 1;
            }
        } else {
            sddmm_yrows = sddmm_xrows;
        }
    }
    // --reduce: the dimension and the op (pem_binop; default: the semiring's additive op)
    int reduce_dim = -1, reduce_op = add_ops[semiring];
    if (reduce_spec) {
        const char *clash = ngpu > 0 ? "--gpus" : power ? "--power" : nullptr;
        if (clash) {
            printf("--reduce does not combine with %s. Exiting.\n", clash);
            return 1;
        }
        const char *colon = strchr(reduce_spec, ':');
        const std::string dim = colon ? std::string(reduce_spec, (size_t)(colon - reduce_spec)) : std::string(reduce_spec);
        reduce_dim = dim == "rows" ? PEM_REDUCE_ROWS : dim == "cols" ? PEM_REDUCE_COLS : -1;
        if (reduce_dim < 0) {
            printf("--reduce %s: unknown dimension %s (rows, cols). Exiting.\n", reduce_spec, dim.c_str());
            return 1;
        }
        if (colon) {
            reduce_op = -1;
            for (int i = 0; i < 6; ++i)
                if (!strcmp(colon + 1, add_op_names[i])) reduce_op = i;
            if (reduce_op < 0) {
                printf("--reduce %s: unknown op %s (plus, times, min, max, lor, land). Exiting.\n", reduce_spec, colon + 1);
                return 1;
            }
        }
    }
    // --bfs: the 1-based source
    long long bfs_src = 0;
    if (bfs_spec) {
        const char *clash = ngpu > 0 ? "--gpus" : power ? "--power" : reduce_spec ? "--reduce" : spmm_path ? "--spmm" : sddmm_path ? "--sddmm" : nullptr;
        if (clash) {
            printf("--bfs does not combine with %s. Exiting.\n", clash);
            return 1;
        }
        char *end = nullptr;
        bfs_src = strtoll(bfs_spec, &end, 10);
        if (end == bfs_spec || *end != '\0' || bfs_src < 1) {
            printf("--bfs %s: want a 1-based vertex number. Exiting.\n", bfs_spec);
            return 1;
        }
    }
    if (ngpu > 0 && mask_path) {
        printf("--gpus does not combine with --mask (masked products run on one device). Exiting.\n");
        return 1;
    }
    if (ngpu > 0) {
        if (fp32 || cache_dir) {
            printf("--gpus does not combine with --fp32 / --cache. Exiting.\n");
            return 1;
        }
        auto conv_start_m = std::chrono::high_resolution_clock::now();
        pem_coo ca, cb;
        memset(&ca, 0, sizeof ca);
        memset(&cb, 0, sizeof cb);
        if (read_input(argv[1], &ca) != 0 || (b_path && read_input(b_path, &cb) != 0)) return 1;
        if (!b_path && !aat && ca.rows != ca.cols) {
            printf("input is rectangular. Only AAt is possible. Exiting.\n");   // spgemm.cu:782-786
            return 1;
        }
        printf("MATRIX A\nfilepath: %s\nRows: %d\nCols: %d\nNnz: %lld\n", argv[1], ca.rows, ca.cols, (long long)ca.nnz);
        MultiResult mr;
        int rc = run_multi(ngpu, ca, b_path ? &cb : nullptr, aat, save || out_path, WARMUP, REPEAT, fastest, conv_start_m, mr, tune_split, nchunks);
        if (rc == 0) {
            const double kernel = mr.step1 + mr.step2 + mr.step3, malloc_ms = mr.total - kernel;
            const double gflops = mr.total > 0 ? (double)mr.flop * 2.0 / (mr.total * 1e6) : 0.0;
            const double gflops_x = mr.total + mr.gather_ms > 0 ? (double)mr.flop * 2.0 / ((mr.total + mr.gather_ms) * 1e6) : 0.0;
            const double ratio = mr.nnz_c ? (double)mr.flop / (double)mr.nnz_c : 0.0;
            printf("\n%d GPUs, row blocks of A balanced on tile-level products, B replicated\nwarm up %d time\naverage over %d iterations\n\n", ngpu, WARMUP, REPEAT);
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
            const double b_alg = 12.0 * ((double)ca.nnz + (double)(b_path ? cb.nnz : ca.nnz) + (double)mr.nnz_c) + 4.0 * 3.0 * ((double)ca.rows + 1);
            const double frac_kernel = kernel > 0 ? b_alg / (kernel * 1e-3) / (8.0e12 * ngpu) : 0.0;
            const double frac_total = mr.total > 0 ? b_alg / (mr.total * 1e-3) / (8.0e12 * ngpu) : 0.0;
            std::string path = argv[1];
            size_t slash = path.find_last_of('/');
            std::string stem = slash == std::string::npos ? path : path.substr(slash + 1);
            if (stem.size() > 4 && stem.compare(stem.size() - 4, 4, ".mtx") == 0) stem.resize(stem.size() - 4);
            pem_csv_record rec = {stem.c_str(), mr.flop, mr.nnz_c, ratio, mr.a_conv_kernel_ms, mr.b_conv_kernel_ms, mr.conv_ms,
                                  mr.step1, mr.step2, mr.step3, mr.total, kernel, malloc_ms, gflops};
            char extra[320];
            // columns 15..: gpus, B_alg, roofline fraction (kernel, total), C tiles, live pairs, first-pass ms, gather ms (sequential),
            // chunks per rank, chunked pass ms, transfers still in flight after it ms, split-tuning rounds, slowest rank before / after (ms)
            snprintf(extra, sizeof extra, "%d,%.0f,%.4f,%.4f,%lld,%lld,%.2f,%.2f,%d,%.2f,%.2f,%d,%.3f,%.3f", ngpu, b_alg, frac_kernel, frac_total,
                     (long long)mr.ntiles_c, (long long)mr.npairs, mr.cold, mr.gather_ms, mr.chunks, mr.chunk_pass_ms, mr.chunk_tail_ms, mr.tune_rounds,
                     mr.tune_first_max, mr.tune_best_max);
            const char *csv = getenv("PEM_CSV") ? getenv("PEM_CSV") : "./pemspgemm_benchmark_result.csv";
            if (pem_csv_append(csv, &rec, extra) != 0) fprintf(stderr, "pemspgemm: %s\n", pem_host_last_error());
            if (!save) {
                printf("Not saving results. Exiting.\n");
            } else {
                const char *dir = getenv("PEM_RESULT_DIR") ? getenv("PEM_RESULT_DIR") : "/tmp";
                std::vector<int32_t> rows((size_t)mr.nnz_c);
                for (int64_t r = 0; r < mr.rows; ++r)   // sorted (row, col) order = CSR order (spgemm.cu:1516-1519)
                    for (int32_t e = mr.rowptr[(size_t)r]; e < mr.rowptr[(size_t)r + 1]; ++e) rows[(size_t)e] = (int32_t)r;
                printf("Saving results to %s/SPGEMM_RESULT_*.txt\n", dir);
                if (pem_write_result_files(dir, mr.nnz_c, rows.data(), mr.colidx.data(), mr.vals.data()) != 0) {
                    fprintf(stderr, "pemspgemm: %s\n", pem_host_last_error());
                    rc = 2;
                }
            }
            if (out_path) {
                if (pem_write_mtx_csr(out_path, (int32_t)mr.rows, mr.cols_b, mr.rowptr.data(), mr.colidx.data(), mr.vals.data(),
                                      "C = A*B by pemspgemm (pem-spgemm_amd), row blocks gathered over RCCL") != 0) {
                    fprintf(stderr, "pemspgemm: %s\n", pem_host_last_error());
                    rc = 2;
                } else {
                    printf("C written to %s\n", out_path);
                }
            }
        }
        printf("CLEANING UP RESOURCES\n\n");
        pem_coo_free(&ca);
        pem_coo_free(&cb);
        return rc;
    }
    pem_ctx *ctx = nullptr;   // device + memory set-up precede the conversion clock, as in the reference (spgemm.cu:730-758)
    CHECK(pem_ctx_create(env_int("PEM_DEVICE", 0), &ctx));
    auto conv_start = std::chrono::high_resolution_clock::now();   // spgemm.cu:760: the clock starts before the file is read
    // One tiling = (source file, transposed?).  With --cache it is loaded from <dir>/<stem>.<A|AT>.pemtile when that
    // file was made from the same .mtx (size + mtime), else parsed + converted and then saved there.
    struct Source {
        const char *path;
        pem_coo coo;
        bool read = false;
    };
    Source srcA = {argv[1], {}, false}, srcB = {b_path, {}, false};
    memset(&srcA.coo, 0, sizeof srcA.coo);
    memset(&srcB.coo, 0, sizeof srcB.coo);
    int cache_hits = 0, cache_misses = 0;
    auto make_tiling = [&](Source &src, int transpose, pem_tiled **out) -> int {
        std::string cpath;
        pem_cache_key key;
        memset(&key, 0, sizeof key);
        bool keyed = false;
        if (cache_dir) {
            struct stat st;
            if (stat(src.path, &st) == 0) {
                key.source_size = (uint64_t)st.st_size;
                key.source_mtime_ns = (int64_t)st.st_mtim.tv_sec * 1000000000ll + st.st_mtim.tv_nsec;
                key.transpose = (uint32_t)transpose;
                keyed = true;
                std::string p = src.path;
                size_t sl = p.find_last_of('/');
                std::string stem = sl == std::string::npos ? p : p.substr(sl + 1);
                cpath = std::string(cache_dir) + "/" + stem + (transpose ? ".AT" : ".A") + (fp32 ? ".f32" : "") + ".pemtile";
                pem_status ls = pem_tiled_load(ctx, cpath.c_str(), &key, out);
                if (ls == PEM_OK) {
                    pem_tiled_info li;
                    if (pem_tiled_get_info(*out, &li) == PEM_OK && li.value_bytes == (fp32 ? 4 : 8)) {
                        ++cache_hits;
                        return 0;
                    }
                    pem_tiled_destroy(ctx, *out);   // a file of the other value type under this name: rebuild
                    *out = nullptr;
                    ls = PEM_E_STALE;
                }
                if (ls != PEM_E_IO && ls != PEM_E_STALE) {
                    fprintf(stderr, "pemspgemm: %s\n", pem_last_error());
                    return 2;
                }
                ++cache_misses;   // absent, stale or damaged: rebuild below and overwrite
            }
        }
        if (!src.read) {
            if (read_input(src.path, &src.coo) != 0) return 1;
            src.read = true;
        }
        const pem_coo &m = src.coo;
        pem_status cs;
        if (fp32) {
            std::vector<float> vf((size_t)m.nnz);
            for (int64_t e = 0; e < m.nnz; ++e) vf[(size_t)e] = (float)m.V[e];
            cs = pem_tiled_from_coo_f32(ctx, m.rows, m.cols, m.nnz, m.I, m.J, vf.data(), transpose, out);
        } else {
            cs = pem_tiled_from_coo(ctx, m.rows, m.cols, m.nnz, m.I, m.J, m.V, transpose, out);
        }
        if (cs != PEM_OK) {
            fprintf(stderr, "pemspgemm: conversion of %s failed: %s\n", src.path, pem_last_error());
            return 2;
        }
        if (keyed && pem_tiled_save(ctx, *out, cpath.c_str(), &key) != PEM_OK)
            fprintf(stderr, "pemspgemm: cache not written: %s\n", pem_last_error());   // not fatal
        return 0;
    };
    pem_tiled *A = nullptr, *B = nullptr;
    if (int rc = make_tiling(srcA, 0, &A)) return rc;
    if (b_path) {
        if (int rc = make_tiling(srcB, aat ? 1 : 0, &B)) return rc;
    } else if (aat) {
        if (int rc = make_tiling(srcA, 1, &B)) return rc;
    } else {
        B = A;   // the reference converts the same file twice (spgemm.cu:778-779); one tiling serves both roles here
    }
    pem_tiled_info ia, ib;
    CHECK(pem_tiled_get_info(A, &ia));
    CHECK(pem_tiled_get_info(B, &ib));
    if (ia.cols != ib.rows) {
        if (b_path)
            printf("inner dimensions differ: A is %d x %d, B%s is %d x %d. Exiting.\n", ia.rows, ia.cols, aat ? "^T" : "", ib.rows, ib.cols);
        else
            printf("input is rectangular. Only AAt is possible. Exiting.\n");   // spgemm.cu:782-786
        return 1;
    }
    pem_tiled *Mt = nullptr;   // --mask: M's structure (its values are never read, so it is converted as fp64 whatever --fp32 says)
    pem_coo cm;
    memset(&cm, 0, sizeof cm);
    if (mask_path) {
        if (read_input(mask_path, &cm) != 0) return 1;
        if (cm.rows != ia.rows || cm.cols != ib.cols) {
            printf("mask %s is %d x %d but C = A*B%s is %d x %d. Exiting.\n", mask_path, cm.rows, cm.cols, aat ? "^T" : "", ia.rows, ib.cols);
            pem_coo_free(&cm);
            return 1;
        }
        if (pem_tiled_from_coo(ctx, cm.rows, cm.cols, cm.nnz, cm.I, cm.J, cm.V, 0, &Mt) != PEM_OK) {
            fprintf(stderr, "pemspgemm: conversion of %s failed: %s\n", mask_path, pem_last_error());
            pem_coo_free(&cm);
            return 2;
        }
    }
    pem_tiled *Dt = nullptr;   // --add: D, in the value type of A
    pem_coo cd;
    memset(&cd, 0, sizeof cd);
    if (add_path) {
        if (read_input(add_path, &cd) != 0) return 1;
        if (cd.rows != ia.rows || cd.cols != ib.cols) {
            printf("--add %s is %d x %d but C = A*B%s is %d x %d. Exiting.\n", add_path, cd.rows, cd.cols, aat ? "^T" : "", ia.rows, ib.cols);
            pem_coo_free(&cd);
            return 1;
        }
        pem_status ds;
        if (fp32) {
            std::vector<float> vf((size_t)cd.nnz);
            for (int64_t e = 0; e < cd.nnz; ++e) vf[(size_t)e] = (float)cd.V[e];
            ds = pem_tiled_from_coo_f32(ctx, cd.rows, cd.cols, cd.nnz, cd.I, cd.J, vf.data(), 0, &Dt);
        } else {
            ds = pem_tiled_from_coo(ctx, cd.rows, cd.cols, cd.nnz, cd.I, cd.J, cd.V, 0, &Dt);
        }
        if (ds != PEM_OK) {
            fprintf(stderr, "pemspgemm: conversion of %s failed: %s\n", add_path, pem_last_error());
            pem_coo_free(&cd);
            return 2;
        }
    }
    pem_tiled *Into = nullptr;   // --assign-into: D, in the value type of A
    pem_coo cinto;
    memset(&cinto, 0, sizeof cinto);
    if (assign_into) {
        if (read_input(assign_into, &cinto) != 0) return 1;
        const int dims[2] = {cinto.rows, cinto.cols};
        for (int q = 0; q < 2; ++q)
            for (size_t j = 0; j < assign_idx[q].size(); ++j)
                if (assign_idx[q][j] >= dims[q]) {
                    printf("%s %s: index %zu is %d; %s has %d %s. Exiting.\n", assign_flags[q], assign_paths[q], j + 1, assign_idx[q][j] + 1,
                           assign_into, dims[q], q ? "columns" : "rows");
                    pem_coo_free(&cinto);
                    return 1;
                }
        pem_status ds;
        if (fp32) {
            std::vector<float> vf((size_t)cinto.nnz);
            for (int64_t e = 0; e < cinto.nnz; ++e) vf[(size_t)e] = (float)cinto.V[e];
            ds = pem_tiled_from_coo_f32(ctx, cinto.rows, cinto.cols, cinto.nnz, cinto.I, cinto.J, vf.data(), 0, &Into);
        } else {
            ds = pem_tiled_from_coo(ctx, cinto.rows, cinto.cols, cinto.nnz, cinto.I, cinto.J, cinto.V, 0, &Into);
        }
        if (ds != PEM_OK) {
            fprintf(stderr, "pemspgemm: conversion of %s failed: %s\n", assign_into, pem_last_error());
            pem_coo_free(&cinto);
            return 2;
        }
    }
    if (fp32) printf("value type: fp32 (the reference computes in fp64)\n");
    printf("MATRIX A\nfilepath: %s\nRows: %d\nCols: %d\nNnz: %lld\n", argv[1], ia.rows, ia.cols, (long long)ia.nnz);   // spgemm.cu:794-806
    printf("MATRIX B\nfilepath: %s\nRows: %d\nCols: %d\nNnz: %lld\n", b_path ? b_path : argv[1], ib.rows, ib.cols, (long long)ib.nnz);
    if (cache_dir) printf("tiled-format cache %s: %d loaded, %d rebuilt\n", cache_dir, cache_hits, cache_misses);
    if (mask_path)
        printf("MASK%s\nfilepath: %s\nRows: %d\nCols: %d\nNnz: %lld\n", mask_complement ? " (complement)" : "", mask_path, cm.rows, cm.cols,
               (long long)cm.nnz);
    double conv_ms = std::chrono::duration<double, std::milli>(std::chrono::high_resolution_clock::now() - conv_start).count();
    // --power K: the first K-2 products run once each; every C becomes the next left operand on the device (pem_tiled_from_cplan),
    // the right operand is always A.  The timed product below is the last one, L * A; its conversion column adds the derived ones.
    pem_tiled *L = A;
    for (int k = 2; k < power; ++k) {
        uint64_t f = 0;
        CHECK(pem_flop_count(ctx, L, A, &f));
        pem_cplan *p = nullptr;
        CHECK(pem_cplan_create(ctx, L, A, 0, -1, &p));
        CHECK(pem_cplan_set_semiring(p, semiring));
        CHECK(pem_spgemm(ctx, p));
        pem_timings t;
        CHECK(pem_get_timings(ctx, &t));
        pem_tiled *next = nullptr;
        CHECK(pem_tiled_from_cplan(ctx, p, 0, &next));
        pem_cplan_info pi;
        pem_tiled_info ni;
        CHECK(pem_cplan_get_info(p, &pi));
        CHECK(pem_tiled_get_info(next, &ni));
        printf("power: A^%d = A^%d * A: flop %llu, C nnz %lld, pass %.2fms, C -> operand %.2fms\n", k, k - 1, (unsigned long long)f,
               (long long)pi.nnz_c, t.spgemm_wall_ms, ni.conv_ms);
        conv_ms += ni.conv_ms;
        pem_cplan_destroy(ctx, p);
        if (L != A) pem_tiled_destroy(ctx, L);
        L = next;
    }
    pem_tiled_info il;
    CHECK(pem_tiled_get_info(L, &il));
    uint64_t flop = 0;
    CHECK(pem_flop_count(ctx, L, B, &flop));   // spgemm.cu:1068-1079

    pem_cplan *plan = nullptr;
    if (Mt)
        CHECK(pem_cplan_create_masked(ctx, A, B, Mt, mask_complement ? PEM_MASK_COMPLEMENT : PEM_MASK_STRUCTURE, 0, -1, &plan));
    else
        CHECK(pem_cplan_create(ctx, L, B, 0, -1, &plan));
    CHECK(pem_cplan_set_semiring(plan, semiring));
    std::vector<double> s1, s2, s3, wall;
    double cold_ms = 0.0;   // the first pass on the plan: every allocation + the three size read-backs (what the reference pays per iteration)
    for (int n = 0; n < WARMUP + REPEAT; ++n) {   // spgemm.cu:1133-1357
        if (n == 0) printf("\nstep1 pemSpGEMM (row-local tile-level expand + sort)\n\nstep2 pemSpGEMM\n\nstep3 pemSpGEMM\n\n\n");
        CHECK(pem_spgemm(ctx, plan));
        pem_timings t;
        CHECK(pem_get_timings(ctx, &t));
        if (n == 0) cold_ms = t.spgemm_wall_ms;
        if (n >= WARMUP) {
            s1.push_back(t.step1_ms);
            s2.push_back(t.step2_ms);
            s3.push_back(t.step3_ms);
            wall.push_back(t.spgemm_wall_ms);
        }
    }
    auto pick = [&](const std::vector<double> &v, size_t idx) {
        if (v.empty()) return 0.0;
        if (fastest) return v[idx];
        double s = 0;
        for (double x : v) s += x;
        return s / (double)v.size();
    };
    size_t fidx = 0;
    if (fastest && !wall.empty()) {
        fidx = (size_t)(std::min_element(wall.begin(), wall.end()) - wall.begin());
        printf("fidx: %zu\n\n", fidx);
    } else {
        printf("warm up %d time\naverage over %d iterations\n\n", WARMUP, REPEAT);
    }
    const double step1 = pick(s1, fidx), step2 = pick(s2, fidx), step3 = pick(s3, fidx), total = pick(wall, fidx);
    const double kernel = step1 + step2 + step3, malloc_ms = total - kernel;   // spgemm.cu:1353-1354
    pem_cplan_info ci;
    CHECK(pem_cplan_get_info(plan, &ci));
    const double gflops = total > 0 ? (double)flop * 2.0 / (total * 1e6) : 0.0;   // spgemm.cu:1403
    const double ratio = ci.nnz_c ? (double)flop / (double)ci.nnz_c : 0.0;       // spgemm.cu:1404

    printf("<---Program done--->\n");   // spgemm.cu:1406-1422
    printf("Matrix A CSR to tile kernel took---------%.2fms\n", ia.conv_tile_kernel_ms);
    printf("Matrix B CSR to tile kernel took---------%.2fms\n", ib.conv_tile_kernel_ms);
    printf("total conversion overhead----------------%.2fms\n\n", conv_ms);
    printf("step1 - High Level Multiplication took---%.2fms\n", step1);
    printf("step2 - Allocating C took----------------%.2fms\n", step2);
    printf("step3 - Accumulation took----------------%.2fms\n\n", step3);
    printf("pemSpGEMM took %.2fms ----- GFlops: %.2f\nKernel time %.2fms\nmalloc time %.2fms\n", total, gflops, kernel, malloc_ms);
    printf("first pass (allocations + size read-backs) %.2fms; the passes above re-use the plan's buffers and sizes\n", cold_ms);
    printf("Flop count: %llu\n\n", (unsigned long long)flop);
    if (Mt) printf("masked product C<%sM>: the flop count and GFlops above count the unmasked product A*B\n", mask_complement ? "!" : "");
    if (semiring != PEM_SEMIRING_PLUS_TIMES)
        printf("semiring %s: step 3 reduced under it; the flop count and GFlops above count the tile product's multiply-adds\n", semiring_names[semiring]);
    printf("C tiles: %lld\n", (long long)ci.ntiles_c);
    printf("C nnz: %lld\n", (long long)ci.nnz_c);
    if (power >= 2)
        printf("power: A^%d = A^%d * A: flop %llu, C nnz %lld, pass %.2fms\n", power, power - 1, (unsigned long long)flop, (long long)ci.nnz_c, total);
    printf("Compression ratio %.2f\n", ratio);
    // roofline bookkeeping
    const double b_alg = 12.0 * ((double)il.nnz + (double)ib.nnz + (double)ci.nnz_c) + 4.0 * ((double)ia.rows + 1) + 4.0 * ((double)ib.rows + 1) +
                         4.0 * ((double)ia.rows + 1);
    const double frac_kernel = kernel > 0 ? b_alg / (kernel * 1e-3) / 8.0e12 : 0.0, frac_total = total > 0 ? b_alg / (total * 1e-3) / 8.0e12 : 0.0;
    printf("B_alg %.0f bytes; HBM roofline fraction (8 TB/s): kernel %.4f, total %.4f\n", b_alg, frac_kernel, frac_total);

    // CSV (spgemm.cu:1424-1450); matrix name = file stem (the reference's regex needs a '/' in the path)
    std::string path = argv[1];
    size_t slash = path.find_last_of('/');
    std::string stem = slash == std::string::npos ? path : path.substr(slash + 1);
    if (stem.size() > 4 && stem.compare(stem.size() - 4, 4, ".mtx") == 0) stem.resize(stem.size() - 4);
    pem_csv_record rec = {stem.c_str(), flop, ci.nnz_c, ratio, ia.conv_tile_kernel_ms, ib.conv_tile_kernel_ms, conv_ms,
                          step1, step2, step3, total, kernel, malloc_ms, gflops};
    char extra[256];
    // columns 15..: gpus, B_alg, roofline fraction (kernel, total), C tiles, live pairs, first-pass ms, gather ms
    snprintf(extra, sizeof extra, "1,%.0f,%.4f,%.4f,%lld,%lld,%.2f,0.00", b_alg, frac_kernel, frac_total, (long long)ci.ntiles_c, (long long)ci.npairs,
             cold_ms);
    const char *csv = getenv("PEM_CSV") ? getenv("PEM_CSV") : "./pemspgemm_benchmark_result.csv";
    if (pem_csv_append(csv, &rec, extra) != 0) fprintf(stderr, "pemspgemm: %s\n", pem_host_last_error());

    pem_tiled *Sum = nullptr;   // --add: alpha*C (+) beta*D
    if (Dt) {
        auto a0 = std::chrono::high_resolution_clock::now();
        pem_tiled *Ct = nullptr;
        CHECK(pem_tiled_from_cplan(ctx, plan, 0, &Ct));
        const int op = add_ops[semiring];
        CHECK(pem_tiled_ewise(ctx, Ct, Dt, PEM_EWISE_UNION, op, add_alpha, add_beta, &Sum));
        const double add_ms = std::chrono::duration<double, std::milli>(std::chrono::high_resolution_clock::now() - a0).count();
        pem_tiled_info si, ct;
        CHECK(pem_tiled_get_info(Sum, &si));
        CHECK(pem_tiled_get_info(Ct, &ct));
        printf("add: C = %g*(A*B) %s %g*D over the union: C -> tiling %.2fms, ewise %.2fms, total %.2fms, nnz %lld\n", add_alpha, add_op_names[op],
               add_beta, ct.conv_ms, si.conv_ms, add_ms, (long long)si.nnz);
        pem_tiled_destroy(ctx, Ct);
    }
    pem_tiled *Sel = nullptr;   // --select: the entries of C (or of the sum) that satisfy the op
    if (select_op >= 0) {
        auto s0 = std::chrono::high_resolution_clock::now();
        pem_tiled *Src = Sum, *Ct = nullptr;
        if (!Src) {
            CHECK(pem_tiled_from_cplan(ctx, plan, 0, &Ct));
            Src = Ct;
        }
        CHECK(pem_tiled_select(ctx, Src, select_op, select_thunk, &Sel));
        const double sel_total_ms = std::chrono::duration<double, std::milli>(std::chrono::high_resolution_clock::now() - s0).count();
        pem_tiled_info si, src;
        CHECK(pem_tiled_get_info(Sel, &si));
        CHECK(pem_tiled_get_info(Src, &src));
        printf("select: %s:%g of %s: select %.2fms, total %.2fms, nnz %lld of %lld kept\n", select_names[select_op], select_thunk,
               Sum ? "the sum" : "C", si.conv_ms, sel_total_ms, (long long)si.nnz, (long long)src.nnz);
        if (Ct) pem_tiled_destroy(ctx, Ct);
    }
    pem_tiled *Ext = nullptr;   // --extract-rows / --extract-cols: R(I, J) of C, of the sum or of the selection
    if (extract_paths[0] || extract_paths[1]) {
        auto x0 = std::chrono::high_resolution_clock::now();
        pem_tiled *Src = Sel ? Sel : Sum, *Ct = nullptr;
        if (!Src) {
            CHECK(pem_tiled_from_cplan(ctx, plan, 0, &Ct));
            Src = Ct;
        }
        pem_tiled_info xi, src;
        CHECK(pem_tiled_get_info(Src, &src));
        const int dims[2] = {src.rows, src.cols};
        for (int q = 0; q < 2; ++q)
            for (size_t j = 0; j < extract_idx[q].size(); ++j)
                if (extract_idx[q][j] >= dims[q]) {
                    printf("%s %s: index %zu is %d; the result has %d %s. Exiting.\n", extract_flags[q], extract_paths[q], j + 1,
                           extract_idx[q][j] + 1, dims[q], q ? "columns" : "rows");
                    if (Ct) pem_tiled_destroy(ctx, Ct);
                    return 1;
                }
        CHECK(pem_tiled_extract(ctx, Src, extract_paths[0] ? extract_idx[0].data() : nullptr, (int64_t)extract_idx[0].size(),
                                extract_paths[1] ? extract_idx[1].data() : nullptr, (int64_t)extract_idx[1].size(), &Ext));
        const double ext_total_ms = std::chrono::duration<double, std::milli>(std::chrono::high_resolution_clock::now() - x0).count();
        CHECK(pem_tiled_get_info(Ext, &xi));
        printf("extract: %s x %s of %s: extract %.2fms, total %.2fms, %d x %d, nnz %lld from %lld\n",
               extract_paths[0] ? std::to_string(extract_idx[0].size()).append(" rows").c_str() : "all rows",
               extract_paths[1] ? std::to_string(extract_idx[1].size()).append(" columns").c_str() : "all columns",
               Sel ? "the selection" : Sum ? "the sum" : "C", xi.conv_ms, ext_total_ms, xi.rows, xi.cols, (long long)xi.nnz, (long long)src.nnz);
        if (Ct) pem_tiled_destroy(ctx, Ct);
    }
    pem_tiled *Asg = nullptr;   // --assign-into: D with D(I, J) = R, R being C, the sum, the selection or the extract
    if (Into) {
        auto g0 = std::chrono::high_resolution_clock::now();
        pem_tiled *Src = Ext ? Ext : Sel ? Sel : Sum, *Ct = nullptr;
        if (!Src) {
            CHECK(pem_tiled_from_cplan(ctx, plan, 0, &Ct));
            Src = Ct;
        }
        pem_tiled_info gi, src, di;
        CHECK(pem_tiled_get_info(Src, &src));
        CHECK(pem_tiled_get_info(Into, &di));
        const long long want_r = assign_paths[0] ? (long long)assign_idx[0].size() : di.rows;
        const long long want_c = assign_paths[1] ? (long long)assign_idx[1].size() : di.cols;
        if (src.rows != want_r || src.cols != want_c) {
            printf("--assign-into %s: the result is %d x %d but the region is %lld x %lld (%s is %d x %d). Exiting.\n", assign_into, src.rows, src.cols,
                   want_r, want_c, assign_into, di.rows, di.cols);
            if (Ct) pem_tiled_destroy(ctx, Ct);
            return 1;
        }
        CHECK(pem_tiled_assign(ctx, Into, Src, assign_paths[0] ? assign_idx[0].data() : nullptr, (int64_t)assign_idx[0].size(),
                               assign_paths[1] ? assign_idx[1].data() : nullptr, (int64_t)assign_idx[1].size(), assign_accum, &Asg));
        const double asg_total_ms = std::chrono::duration<double, std::milli>(std::chrono::high_resolution_clock::now() - g0).count();
        CHECK(pem_tiled_get_info(Asg, &gi));
        printf("assign: %s into %s at %s x %s%s%s: assign %.2fms, total %.2fms, %d x %d, nnz %lld (D %lld, the result %lld)\n",
               Ext ? "the extract" : Sel ? "the selection" : Sum ? "the sum" : "C", assign_into,
               assign_paths[0] ? std::to_string(assign_idx[0].size()).append(" rows").c_str() : "all rows",
               assign_paths[1] ? std::to_string(assign_idx[1].size()).append(" columns").c_str() : "all columns",
               assign_accum == PEM_ACCUM_NONE ? "" : ", accum ", assign_accum == PEM_ACCUM_NONE ? "" : add_op_names[assign_accum], gi.conv_ms,
               asg_total_ms, gi.rows, gi.cols, (long long)gi.nnz, (long long)di.nnz, (long long)src.nnz);
        if (Ct) pem_tiled_destroy(ctx, Ct);
    }
    pem_tiled *const Last = Asg ? Asg : Ext ? Ext : Sel ? Sel : Sum;   // the final result when it is a tiling, and what the lines below call it
    const char *const last_name = Asg ? "the assigned matrix" : Ext ? "the extract" : Sel ? "the selection" : Sum ? "the sum" : "C";

    std::vector<double> red;   // --reduce: the vector, on the host
    if (reduce_dim >= 0) {
        pem_tiled *Src = Last, *Ct = nullptr;
        if (!Src) {
            CHECK(pem_tiled_from_cplan(ctx, plan, 0, &Ct));
            Src = Ct;
        }
        pem_tiled_info si;
        CHECK(pem_tiled_get_info(Src, &si));
        const size_t n = (size_t)(reduce_dim == PEM_REDUCE_COLS ? si.cols : si.rows);
        const size_t vb = fp32 ? 4 : 8;
        void *dy = nullptr;
        if (hipMalloc(&dy, vb * n + 8) != hipSuccess) {
            fprintf(stderr, "pemspgemm: --reduce: device allocation of %zu values failed\n", n);
            return 2;
        }
        CHECK(pem_ctx_synchronize(ctx));
        auto r0 = std::chrono::high_resolution_clock::now();
        CHECK(fp32 ? pem_tiled_reduce_f32(ctx, Src, reduce_op, reduce_dim, (float *)dy, 0) : pem_tiled_reduce(ctx, Src, reduce_op, reduce_dim, (double *)dy, 0));
        CHECK(pem_ctx_synchronize(ctx));
        const double red_ms = std::chrono::duration<double, std::milli>(std::chrono::high_resolution_clock::now() - r0).count();
        red.resize(n);
        if (fp32) {
            std::vector<float> f(n);
            if (n && hipMemcpy(f.data(), dy, 4 * n, hipMemcpyDeviceToHost) != hipSuccess) return 2;
            for (size_t i = 0; i < n; ++i) red[i] = f[i];
        } else if (n && hipMemcpy(red.data(), dy, 8 * n, hipMemcpyDeviceToHost) != hipSuccess) {
            return 2;
        }
        (void)hipFree(dy);
        double sum = 0.0;
        for (double v : red) sum += v;
        printf("reduce: %s %s of %s: reduce %.3fms, %zu values, host sum %.17g\n", reduce_dim == PEM_REDUCE_COLS ? "cols" : "rows",
               add_op_names[reduce_op], last_name, red_ms, n, sum);
        if (Ct) pem_tiled_destroy(ctx, Ct);
    }

    std::vector<int32_t> bfs_levels;   // --bfs: the levels, on the host
    if (bfs_spec) {
        pem_tiled *Src = Last, *Ct = nullptr;
        if (!Src) {
            CHECK(pem_tiled_from_cplan(ctx, plan, 0, &Ct));
            Src = Ct;
        }
        pem_tiled_info si;
        CHECK(pem_tiled_get_info(Src, &si));
        if (si.rows != si.cols || bfs_src > si.rows) {
            if (si.rows != si.cols)
                printf("--bfs %s: %s is %d x %d; a search needs a square matrix. Exiting.\n", bfs_spec, last_name, si.rows, si.cols);
            else
                printf("--bfs %s: %s has %d vertices. Exiting.\n", bfs_spec, last_name, si.rows);
            if (Ct) pem_tiled_destroy(ctx, Ct);
            return 1;
        }
        const size_t n = (size_t)si.rows;
        int32_t *dl = nullptr;
        if (hipMalloc((void **)&dl, 4 * n + 8) != hipSuccess) {
            fprintf(stderr, "pemspgemm: --bfs: device allocation of %zu levels failed\n", n);
            return 2;
        }
        CHECK(pem_ctx_synchronize(ctx));
        int32_t depth = 0;
        int64_t reached = 0;
        auto b0 = std::chrono::high_resolution_clock::now();
        CHECK(pem_tiled_bfs(ctx, Src, (int64_t)(bfs_src - 1), 0, dl, &depth, &reached));
        const double bfs_ms = std::chrono::duration<double, std::milli>(std::chrono::high_resolution_clock::now() - b0).count();
        bfs_levels.resize(n);
        if (hipMemcpy(bfs_levels.data(), dl, 4 * n, hipMemcpyDeviceToHost) != hipSuccess) return 2;
        (void)hipFree(dl);
        printf("bfs: from %lld over %s: depth %d, reached %lld of %zu, bfs %.3fms\n", bfs_src, last_name, depth, (long long)reached, n, bfs_ms);
        if (Ct) pem_tiled_destroy(ctx, Ct);
    }

    std::vector<double> spmm_y;   // --spmm: Y, row-major, on the host
    int64_t spmm_ny = 0;
    if (spmm_path) {
        pem_tiled *Src = Last, *Ct = nullptr;
        if (!Src) {
            CHECK(pem_tiled_from_cplan(ctx, plan, 0, &Ct));
            Src = Ct;
        }
        pem_tiled_info si;
        CHECK(pem_tiled_get_info(Src, &si));
        if (spmm_rows != si.cols) {
            printf("--spmm %s: X has %lld rows; the result has %d columns. Exiting.\n", spmm_path, (long long)spmm_rows, si.cols);
            if (Ct) pem_tiled_destroy(ctx, Ct);
            return 1;
        }
        const int64_t k = spmm_k, ld = k > 1 ? k : 1;
        spmm_ny = si.rows;
        const size_t vb = fp32 ? 4 : 8, nxv = (size_t)spmm_rows * (size_t)ld, nyv = (size_t)spmm_ny * (size_t)ld;
        void *dx = nullptr, *dy = nullptr;
        if (hipMalloc(&dx, vb * nxv + 8) != hipSuccess || hipMalloc(&dy, vb * nyv + 8) != hipSuccess) {
            fprintf(stderr, "pemspgemm: --spmm: device allocation failed\n");
            return 2;
        }
        if (fp32) {
            std::vector<float> xf(spmm_x.begin(), spmm_x.end());
            if (nxv && hipMemcpy(dx, xf.data(), 4 * nxv, hipMemcpyHostToDevice) != hipSuccess) return 2;
        } else if (nxv && hipMemcpy(dx, spmm_x.data(), 8 * nxv, hipMemcpyHostToDevice) != hipSuccess) {
            return 2;
        }
        CHECK(pem_ctx_synchronize(ctx));
        auto m0 = std::chrono::high_resolution_clock::now();
        CHECK(fp32 ? pem_tiled_spmm_f32(ctx, Src, semiring, 0, k, (const float *)dx, ld, (float *)dy, ld, 0)
                   : pem_tiled_spmm(ctx, Src, semiring, 0, k, (const double *)dx, ld, (double *)dy, ld, 0));
        CHECK(pem_ctx_synchronize(ctx));
        const double spmm_ms = std::chrono::duration<double, std::milli>(std::chrono::high_resolution_clock::now() - m0).count();
        spmm_y.resize(nyv);
        if (fp32) {
            std::vector<float> f(nyv);
            if (nyv && hipMemcpy(f.data(), dy, 4 * nyv, hipMemcpyDeviceToHost) != hipSuccess) return 2;
            for (size_t i = 0; i < nyv; ++i) spmm_y[i] = f[i];
        } else if (nyv && hipMemcpy(spmm_y.data(), dy, 8 * nyv, hipMemcpyDeviceToHost) != hipSuccess) {
            return 2;
        }
        (void)hipFree(dx);
        (void)hipFree(dy);
        double sum = 0.0;
        for (double v : spmm_y) sum += v;
        printf("spmm: Y = %s (%s) X: spmm %.3fms, k %lld, %lld x %lld values, host sum %.17g\n", last_name,
               semiring_names[semiring], spmm_ms, (long long)k, (long long)spmm_ny, (long long)k, sum);
        if (Ct) pem_tiled_destroy(ctx, Ct);
    }

    // --sddmm: the final result's pattern with the values of X Y^T sampled there; its CSR export serves --out and the COO files
    pem_tiled *Sd = nullptr;
    std::vector<int32_t> sd_rp, sd_ci;
    std::vector<double> sd_v;
    if (sddmm_path) {
        pem_tiled *Src = Last, *Ct = nullptr;
        if (!Src) {
            CHECK(pem_tiled_from_cplan(ctx, plan, 0, &Ct));
            Src = Ct;
        }
        pem_tiled_info si;
        CHECK(pem_tiled_get_info(Src, &si));
        if (sddmm_xrows != si.rows || sddmm_yrows != si.cols) {
            if (sddmm_xrows != si.rows)
                printf("--sddmm %s: X has %lld rows; the result has %d rows. Exiting.\n", sddmm_path, (long long)sddmm_xrows, si.rows);
            else
                printf("--sddmm%s %s: Y has %lld rows; the result has %d columns. Exiting.\n", sddmm_y_path ? "-y" : "",
                       sddmm_y_path ? sddmm_y_path : sddmm_path, (long long)sddmm_yrows, si.cols);
            if (Ct) pem_tiled_destroy(ctx, Ct);
            return 1;
        }
        const int64_t k = sddmm_k, ld = k > 1 ? k : 1;
        const size_t vb = fp32 ? 4 : 8, nxv = (size_t)sddmm_xrows * (size_t)ld, nyv = sddmm_y_path ? (size_t)sddmm_yrows * (size_t)ld : 0;
        void *dx = nullptr, *dy = nullptr;
        if (hipMalloc(&dx, vb * nxv + 8) != hipSuccess || (sddmm_y_path && hipMalloc(&dy, vb * nyv + 8) != hipSuccess)) {
            fprintf(stderr, "pemspgemm: --sddmm: device allocation failed\n");
            return 2;
        }
        const std::vector<double> *hv[2] = {&sddmm_x, &sddmm_y};
        void *dv[2] = {dx, dy};
        const size_t nv[2] = {nxv, nyv};
        for (int q = 0; q < 2; ++q) {
            if (!nv[q]) continue;
            if (fp32) {
                std::vector<float> f(hv[q]->begin(), hv[q]->end());
                if (hipMemcpy(dv[q], f.data(), 4 * nv[q], hipMemcpyHostToDevice) != hipSuccess) return 2;
            } else if (hipMemcpy(dv[q], hv[q]->data(), 8 * nv[q], hipMemcpyHostToDevice) != hipSuccess) {
                return 2;
            }
        }
        if (!sddmm_y_path) dy = dx;   // Y = X: the same pointer
        CHECK(pem_ctx_synchronize(ctx));
        auto m0 = std::chrono::high_resolution_clock::now();
        CHECK(fp32 ? pem_tiled_sddmm_f32(ctx, Src, semiring, k, (const float *)dx, ld, (const float *)dy, ld, &Sd)
                   : pem_tiled_sddmm(ctx, Src, semiring, k, (const double *)dx, ld, (const double *)dy, ld, &Sd));
        const double sd_ms = std::chrono::duration<double, std::milli>(std::chrono::high_resolution_clock::now() - m0).count();
        if (sddmm_y_path) (void)hipFree(dy);
        (void)hipFree(dx);
        CHECK(pem_tiled_get_info(Sd, &si));
        sd_rp.resize((size_t)si.rows + 1);
        sd_ci.resize((size_t)si.nnz);
        sd_v.resize((size_t)si.nnz);
        int64_t nnz = 0;
        if (fp32) {
            std::vector<float> vf((size_t)si.nnz);
            CHECK(pem_tiled_export_csr_f32(ctx, Sd, &nnz, sd_rp.data(), sd_ci.data(), vf.data()));
            for (size_t e = 0; e < vf.size(); ++e) sd_v[e] = vf[e];
        } else {
            CHECK(pem_tiled_export_csr(ctx, Sd, &nnz, sd_rp.data(), sd_ci.data(), sd_v.data()));
        }
        double sum = 0.0;
        for (double v : sd_v) sum += v;
        printf("sddmm: R = pattern(%s) o (X %s^T) (%s): sddmm %.3fms, k %lld, nnz %lld, host sum %.17g\n", last_name,
               sddmm_y_path ? "Y" : "X", semiring_names[semiring], sd_ms, (long long)k, (long long)si.nnz, sum);
        if (Ct) pem_tiled_destroy(ctx, Ct);
    }

    int rc = 0;
    if (!save) {
        printf("Not saving results. Exiting.\n");   // spgemm.cu:1487
    } else if (Sd) {   // the sampled product's entries, sorted by (row, column): its CSR export is that order
        const char *dir = getenv("PEM_RESULT_DIR") ? getenv("PEM_RESULT_DIR") : "/tmp";
        std::vector<int32_t> rows(sd_ci.size());
        for (size_t i = 0; i + 1 < sd_rp.size(); ++i)
            for (int32_t e = sd_rp[i]; e < sd_rp[i + 1]; ++e) rows[(size_t)e] = (int32_t)i;
        printf("Saving results to %s/SPGEMM_RESULT_*.txt\n", dir);
        if (pem_write_result_files(dir, (int64_t)sd_ci.size(), rows.data(), sd_ci.data(), sd_v.data()) != 0) {
            fprintf(stderr, "pemspgemm: %s\n", pem_host_last_error());
            rc = 2;
        }
    } else if (Asg) {   // the assigned matrix's entries, sorted by (row, column): its CSR export is that order
        const char *dir = getenv("PEM_RESULT_DIR") ? getenv("PEM_RESULT_DIR") : "/tmp";
        pem_tiled_info gi;
        CHECK(pem_tiled_get_info(Asg, &gi));
        std::vector<int32_t> rp((size_t)gi.rows + 1), rows((size_t)gi.nnz), cols((size_t)gi.nnz);
        std::vector<double> vals((size_t)gi.nnz);
        int64_t nnz = 0;
        if (fp32) {
            std::vector<float> vf((size_t)gi.nnz);
            CHECK(pem_tiled_export_csr_f32(ctx, Asg, &nnz, rp.data(), cols.data(), vf.data()));
            for (size_t e = 0; e < vf.size(); ++e) vals[e] = vf[e];
        } else {
            CHECK(pem_tiled_export_csr(ctx, Asg, &nnz, rp.data(), cols.data(), vals.data()));
        }
        for (size_t i = 0; i + 1 < rp.size(); ++i)
            for (int32_t e = rp[i]; e < rp[i + 1]; ++e) rows[(size_t)e] = (int32_t)i;
        printf("Saving results to %s/SPGEMM_RESULT_*.txt\n", dir);
        if (pem_write_result_files(dir, nnz, rows.data(), cols.data(), vals.data()) != 0) {
            fprintf(stderr, "pemspgemm: %s\n", pem_host_last_error());
            rc = 2;
        }
    } else {
        const char *dir = getenv("PEM_RESULT_DIR") ? getenv("PEM_RESULT_DIR") : "/tmp";
        std::vector<int32_t> rows((size_t)ci.nnz_c), cols((size_t)ci.nnz_c);
        std::vector<double> vals((size_t)ci.nnz_c);
        int64_t nnz = 0;
        if (fp32) {
            std::vector<float> vf((size_t)ci.nnz_c);
            CHECK(pem_c_export_coo_f32(ctx, plan, &nnz, rows.data(), cols.data(), vf.data()));
            for (size_t e = 0; e < vf.size(); ++e) vals[e] = vf[e];
        } else {
            CHECK(pem_c_export_coo(ctx, plan, &nnz, rows.data(), cols.data(), vals.data()));   // spgemm.cu:1493-1543
        }
        pem_timings t;
        CHECK(pem_get_timings(ctx, &t));
        printf("sanitize_C took %.2fms\n", t.export_ms);
        printf("Saving results to %s/SPGEMM_RESULT_*.txt\n", dir);
        if (pem_write_result_files(dir, nnz, rows.data(), cols.data(), vals.data()) != 0) {
            fprintf(stderr, "pemspgemm: %s\n", pem_host_last_error());
            rc = 2;
        }
    }
    pem_tiled *Res = Last;   // the final result when it is a tiling
    const std::string extract_note = !Ext ? std::string()
                                          : std::string(", extract ") + (extract_paths[0] ? std::string("rows ") + extract_paths[0] : std::string()) +
                                                (extract_paths[0] && extract_paths[1] ? ", " : "") +
                                                (extract_paths[1] ? std::string("columns ") + extract_paths[1] : std::string());
    const std::string assign_note = !Asg ? std::string()
                                         : std::string(", assigned into ") + assign_into +
                                               (assign_paths[0] ? std::string(" rows ") + assign_paths[0] : std::string()) +
                                               (assign_paths[1] ? std::string(" columns ") + assign_paths[1] : std::string()) +
                                               (assign_accum == PEM_ACCUM_NONE ? std::string() : std::string(" accum ") + add_op_names[assign_accum]);
    if (out_path && bfs_spec) {   // the levels as a Matrix-Market dense integer array (n x 1)
        FILE *f = fopen(out_path, "w");
        bool ok = f != nullptr;
        if (ok) {
            ok = fprintf(f, "%%%%MatrixMarket matrix array integer general\n%% bfs levels from %lld by pemspgemm (pem-spgemm_amd)\n%zu 1\n", bfs_src,
                         bfs_levels.size()) > 0;
            for (size_t i = 0; ok && i < bfs_levels.size(); ++i) ok = fprintf(f, "%d\n", bfs_levels[i]) > 0;
            ok = fclose(f) == 0 && ok;
        }
        if (!ok) {
            fprintf(stderr, "pemspgemm: --out %s: cannot write the levels\n", out_path);
            rc = 2;
        } else {
            printf("levels written to %s\n", out_path);
        }
    } else if (out_path && spmm_path) {   // Y as a Matrix-Market dense array (R.rows x k, values column by column)
        FILE *f = fopen(out_path, "w");
        bool ok = f != nullptr;
        const int64_t ld = spmm_k > 1 ? spmm_k : 1;
        if (ok) {
            ok = fprintf(f, "%%%%MatrixMarket matrix array real general\n%% Y = R X (%s) by pemspgemm (pem-spgemm_amd)\n%lld %lld\n",
                         semiring_names[semiring], (long long)spmm_ny, (long long)spmm_k) > 0;
            for (int64_t c = 0; ok && c < spmm_k; ++c)
                for (int64_t i = 0; ok && i < spmm_ny; ++i) ok = fprintf(f, fp32 ? "%.9g\n" : "%.17g\n", spmm_y[(size_t)(i * ld + c)]) > 0;
            ok = fclose(f) == 0 && ok;
        }
        if (!ok) {
            fprintf(stderr, "pemspgemm: --out %s: cannot write Y\n", out_path);
            rc = 2;
        } else {
            printf("Y written to %s\n", out_path);
        }
    } else if (out_path && reduce_dim >= 0) {   // the reduced vector as a Matrix-Market dense array (n x 1)
        FILE *f = fopen(out_path, "w");
        bool ok = f != nullptr;
        if (ok) {
            ok = fprintf(f, "%%%%MatrixMarket matrix array real general\n%% reduce %s of C = A*B (%s) by pemspgemm (pem-spgemm_amd)\n%zu 1\n",
                         reduce_spec, semiring_names[semiring], red.size()) > 0;
            for (size_t i = 0; ok && i < red.size(); ++i) ok = fprintf(f, fp32 ? "%.9g\n" : "%.17g\n", red[i]) > 0;
            ok = fclose(f) == 0 && ok;
        }
        if (!ok) {
            fprintf(stderr, "pemspgemm: --out %s: cannot write the vector\n", out_path);
            rc = 2;
        } else {
            printf("vector written to %s\n", out_path);
        }
    } else if (out_path && Sd) {   // the sampled product as a Matrix-Market file
        pem_tiled_info si;
        CHECK(pem_tiled_get_info(Sd, &si));
        std::string comment = std::string("R = pattern(C) o (X Y^T) (") + semiring_names[semiring] + ")";
        if (Sel) comment += std::string(", C after select ") + select_spec;
        comment += extract_note;
        comment += assign_note;
        comment += " by pemspgemm (pem-spgemm_amd)";
        if (pem_write_mtx_csr(out_path, si.rows, si.cols, sd_rp.data(), sd_ci.data(), sd_v.data(), comment.c_str()) != 0) {
            fprintf(stderr, "pemspgemm: %s\n", pem_host_last_error());
            rc = 2;
        } else {
            printf("R written to %s\n", out_path);
        }
    } else if (out_path && Res) {   // the sum and / or the selection as a Matrix-Market file (the tiling's CSR export)
        pem_tiled_info si;
        CHECK(pem_tiled_get_info(Res, &si));
        std::vector<int32_t> rp((size_t)si.rows + 1), cidx((size_t)si.nnz);
        std::vector<double> cv((size_t)si.nnz);
        int64_t nnz = 0;
        if (fp32) {
            std::vector<float> vf((size_t)si.nnz);
            CHECK(pem_tiled_export_csr_f32(ctx, Res, &nnz, rp.data(), cidx.data(), vf.data()));
            for (size_t e = 0; e < vf.size(); ++e) cv[e] = vf[e];
        } else {
            CHECK(pem_tiled_export_csr(ctx, Res, &nnz, rp.data(), cidx.data(), cv.data()));
        }
        std::string comment = Sum ? std::string("C = alpha*A*B + beta*D (") + semiring_names[semiring] + ")" : std::string("C = A*B (") + semiring_names[semiring] + ")";
        if (Sel) comment += std::string(", select ") + select_spec;
        comment += extract_note;
        comment += assign_note;
        comment += " by pemspgemm (pem-spgemm_amd)";
        if (pem_write_mtx_csr(out_path, si.rows, si.cols, rp.data(), cidx.data(), cv.data(), comment.c_str()) != 0) {
            fprintf(stderr, "pemspgemm: %s\n", pem_host_last_error());
            rc = 2;
        } else {
            printf("C written to %s\n", out_path);
        }
    } else if (out_path) {   // C as a Matrix-Market file (CSR export: rows ascending, columns ascending)
        std::vector<int32_t> rp((size_t)(ci.row_end - ci.row_begin) + 1), cidx((size_t)ci.nnz_c);
        std::vector<double> cv((size_t)ci.nnz_c);
        int64_t nnz = 0;
        if (fp32) {
            std::vector<float> vf((size_t)ci.nnz_c);
            CHECK(pem_c_export_csr_f32(ctx, plan, &nnz, rp.data(), cidx.data(), vf.data()));
            for (size_t e = 0; e < vf.size(); ++e) cv[e] = vf[e];
        } else {
            CHECK(pem_c_export_csr(ctx, plan, &nnz, rp.data(), cidx.data(), cv.data()));
        }
        const std::string comment = semiring == PEM_SEMIRING_PLUS_TIMES ? std::string("C = A*B by pemspgemm (pem-spgemm_amd)")
                                                                         : std::string("C = A*B over the ") + semiring_names[semiring] + " semiring by pemspgemm (pem-spgemm_amd)";
        if (pem_write_mtx_csr(out_path, ia.rows, ib.cols, rp.data(), cidx.data(), cv.data(), comment.c_str()) != 0) {
            fprintf(stderr, "pemspgemm: %s\n", pem_host_last_error());
            rc = 2;
        } else {
            printf("C written to %s\n", out_path);
        }
    }
    printf("CLEANING UP RESOURCES\n\n");
    pem_cplan_destroy(ctx, plan);
    if (L != A) pem_tiled_destroy(ctx, L);
    if (Mt) pem_tiled_destroy(ctx, Mt);
    pem_coo_free(&cm);
    if (Sd) pem_tiled_destroy(ctx, Sd);
    if (Asg) pem_tiled_destroy(ctx, Asg);
    if (Into) pem_tiled_destroy(ctx, Into);
    pem_coo_free(&cinto);
    if (Ext) pem_tiled_destroy(ctx, Ext);
    if (Sel) pem_tiled_destroy(ctx, Sel);
    if (Sum) pem_tiled_destroy(ctx, Sum);
    if (Dt) pem_tiled_destroy(ctx, Dt);
    pem_coo_free(&cd);
    if (B != A) pem_tiled_destroy(ctx, B);
    pem_tiled_destroy(ctx, A);
    pem_ctx_destroy(ctx);
    pem_coo_free(&srcA.coo);
    pem_coo_free(&srcB.coo);
    return rc;
}
