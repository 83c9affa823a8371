// main.cpp -- command line of the MI355X SpMV engine.
//
// Keeps the reference's surface (src/main.cpp:139-188): --trace-config/-c, --matrix/-m,
// --spmv-format {coo,coo-atomic,csr,ell,hybrid}, --profile/-p N, --warmup, --flush-caches,
// --verbose/-v, --triad N, one JSON document on stdout, one-line errors on stderr with
// EXIT_FAILURE.  Accepted as well: the README's --csr/--coo/--ell PATH spellings.
// New: --device hip (or --spmv-format hip-csr|hip-coo|hip-ell|hip-hybrid) runs the format on the GPU.
// The default mode of the reference (simulated cache tracing, no --profile) and its libpfm4
// counters are outside this engine and are refused with a message.
#include "kernels/spmv-kernels.hpp"
#include "kernels/triad-kernel.hpp"
#include "matrix/synthetic.hpp"
#include "matrix/matrix-market.hpp"
#include "profile-kernel.hpp"
#include "trace-config.hpp"
#include "util/cpu-budget.hpp"
#include "util/json-ostreambuf.hpp"

#include "spmv_hip_tuning.h" // (spmv_hip.h + the CSR algorithm choice and ctx_info of the CLI)
#include "spmv_hip_multivec.h" // (SPMV_HIP_MV_MAX_VECTORS of --vectors)

#include <argp.h>
#include <locale.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cstdint>
#include <iostream>
#include <memory>
#include <string>
#include <system_error>

char const * argp_program_version = "spmv-cache-trace-hip 1.0 (drop-in for spmv-cache-trace 2.0 --profile)";
char const * argp_program_bug_address = nullptr;

namespace {

enum class KernelType { none, triad, spmv };

struct Arguments
{
    KernelType kernel_type = KernelType::none;
    SpmvFormat format = SpmvFormat::csr;
    bool hip = false;
    std::size_t triad_entries = 0;
    std::string matrix_path;
    std::string write_mtx; // --write-mtx: write the loaded (or generated) matrix to this file and stop
    std::string trace_config;
    int threads = 0;
    int profile = 0;
    bool warmup = false;
    bool flush_caches = false;
    bool list_perf_events = false;
    bool verbose = false;
    bool check = false;
    bool x_uniform = false;
    bool device_given = false;
    bool shortcut = false; // the kernel was chosen with --csr / --coo / --ell PATH
    SpmvOptions spmv;
};

enum Key
{
    key_matrix = 'm',
    key_trace_config = 'c',
    key_profile = 'p',
    key_verbose = 'v',
    key_first_long = 128,
    key_list_perf_events,
    key_warmup,
    key_flush_caches,
    key_triad,
    key_spmv_format,
    key_csr,
    key_coo,
    key_ell,
    key_device,
    key_gpu,
    key_csr_algorithm,
    key_lanes,
    key_expand_symmetric,
    key_matrix_cache,
    key_exact_order,
    key_peer_gather,
    key_fused_peer_store,
    key_pipeline_gather,
    key_balance_entries,
    key_threads,
    key_check,
    key_write_mtx,
    key_synthetic,
    key_x,
    key_gpus,
    key_symmetric,
    key_vectors,
    key_transpose,
    key_f32_values,
    key_compact,
    key_alpha,
    key_beta,
    key_dots,
};

bool parse_count(char const * arg, long long & out)
{
    char * end = nullptr;
    errno = 0;
    out = std::strtoll(arg, &end, 10);
    return errno == 0 && end != arg && *end == '\0' && out >= 0;
}

error_t parse_option(int key, char * arg, argp_state * state)
{
    Arguments & a = *static_cast<Arguments *>(state->input);
    long long n = 0;
    switch (key) {
    case key_matrix: a.matrix_path = arg; break;
    case key_write_mtx: a.write_mtx = arg; break;
    case key_trace_config: a.trace_config = arg; break;
    case key_profile:
        if (!parse_count(arg, n) || n > 1000000000)
            argp_error(state, "Expected 'profile' to be an integer");
        a.profile = (int) n;
        break;
    case key_warmup: a.warmup = true; break;
    case key_flush_caches: a.flush_caches = true; break;
    case key_list_perf_events: a.list_perf_events = true; break;
    case key_verbose: a.verbose = true; break;
    case key_triad:
        if (!parse_count(arg, n))
            argp_error(state, "triad: expected integer");
        a.kernel_type = KernelType::triad;
        a.triad_entries = (std::size_t) n;
        break;
    case key_spmv_format:
        a.kernel_type = KernelType::spmv;
        if (!std::strncmp(arg, "hip-", 4)) {
            a.hip = true;
            a.device_given = true;
            arg += 4;
        }
        if (!std::strcmp(arg, "coo")) a.format = SpmvFormat::coo;
        else if (!std::strcmp(arg, "coo-atomic")) a.format = SpmvFormat::coo_atomic;
        else if (!std::strcmp(arg, "csr")) a.format = SpmvFormat::csr;
        else if (!std::strcmp(arg, "ell")) a.format = SpmvFormat::ell;
        else if (!std::strcmp(arg, "hybrid")) a.format = SpmvFormat::hybrid;
        else if (!std::strcmp(arg, "mkl-csr"))
            argp_error(state, "spmv-format '%s' is not part of this build (choose coo, coo-atomic, csr, ell or hybrid)", arg);
        else argp_error(state, "invalid argument");
        break;
    case key_csr: a.kernel_type = KernelType::spmv; a.format = SpmvFormat::csr; a.matrix_path = arg; a.shortcut = true; break;
    case key_coo: a.kernel_type = KernelType::spmv; a.format = SpmvFormat::coo; a.matrix_path = arg; a.shortcut = true; break;
    case key_ell: a.kernel_type = KernelType::spmv; a.format = SpmvFormat::ell; a.matrix_path = arg; a.shortcut = true; break;
    case key_device:
        if (!std::strcmp(arg, "hip") || !std::strcmp(arg, "gpu")) a.hip = true;
        else if (!std::strcmp(arg, "cpu")) a.hip = false;
        else argp_error(state, "device: expected 'cpu' or 'hip'");
        a.device_given = true;
        break;
    case key_gpu:
        if (!parse_count(arg, n))
            argp_error(state, "gpu: expected a device index");
        a.spmv.device = (int) n;
        break;
    case key_csr_algorithm:
        if (!std::strcmp(arg, "auto")) a.spmv.csr_algorithm = SPMV_HIP_CSR_AUTO;
        else if (!std::strcmp(arg, "scalar")) a.spmv.csr_algorithm = SPMV_HIP_CSR_SCALAR;
        else if (!std::strcmp(arg, "vector")) a.spmv.csr_algorithm = SPMV_HIP_CSR_VECTOR;
        else if (!std::strcmp(arg, "adaptive")) a.spmv.csr_algorithm = SPMV_HIP_CSR_ADAPTIVE;
        else if (!std::strcmp(arg, "wavetile")) a.spmv.csr_algorithm = SPMV_HIP_CSR_WAVETILE;
        else argp_error(state, "csr-algorithm: expected auto, scalar, vector, adaptive or wavetile");
        break;
    case key_lanes:
        if (!parse_count(arg, n))
            argp_error(state, "lanes-per-row: expected integer");
        a.spmv.csr_lanes_per_row = (int) n;
        break;
    case key_expand_symmetric: a.spmv.expand_symmetric = true; break;
    case key_matrix_cache: setenv("SPMV_MATRIX_CACHE", arg, 1); break;
    case key_exact_order: a.spmv.hip_flags |= SPMV_HIP_FLAG_EXACT_ORDER; break;
    case key_peer_gather: a.spmv.hip_flags |= SPMV_HIP_FLAG_PEER_GATHER; break;
    case key_fused_peer_store: a.spmv.hip_flags |= SPMV_HIP_FLAG_FUSED_PEER_STORE; break;
    case key_pipeline_gather: a.spmv.hip_flags |= SPMV_HIP_FLAG_PIPELINE_GATHER; break;
    case key_balance_entries: a.spmv.hip_flags |= SPMV_HIP_FLAG_BALANCE_ENTRIES; break;
    case key_threads:
        if (!parse_count(arg, n) || n < 0 || n > 4096)
            argp_error(state, "threads: expected a positive integer, or 0 for the cores this process may use");
        a.threads = n == 0 ? cpu_budget() : (int) n; // 0: affinity mask capped by the cgroup quota
        break;
    case key_check: a.check = true; break;
    case key_gpus:
        if (!parse_count(arg, n) || n < 1 || n > 64)
            argp_error(state, "gpus: expected a positive integer");
        a.spmv.num_gpus = (int) n;
        break;
    case key_synthetic:
        if (a.kernel_type == KernelType::none)
            a.kernel_type = KernelType::spmv;
        a.matrix_path = std::strncmp(arg, "synthetic:", 10) ? std::string("synthetic:") + arg : std::string(arg);
        break;
    case key_x:
        if (!std::strcmp(arg, "ones")) a.x_uniform = false;
        else if (!std::strcmp(arg, "uniform")) a.x_uniform = true;
        else argp_error(state, "x: expected 'ones' or 'uniform'");
        break;
    case key_symmetric: a.spmv.symmetric = true; break;
    case key_vectors:
        if (!parse_count(arg, n) || n < 1 || n > SPMV_HIP_MV_MAX_VECTORS)
            argp_error(state, "vectors: expected an integer from 1 to 16");
        a.spmv.vectors = (int) n;
        break;
    case key_transpose: a.spmv.transpose = true; break;
    case key_f32_values:
        if (!arg || !std::strcmp(arg, "round")) a.spmv.f32_values = 1;
        else if (!std::strcmp(arg, "exact")) a.spmv.f32_values = 2;
        else argp_error(state, "f32-values: expected 'round' (the default) or 'exact'");
        break;
    case key_compact:
        if (!arg || !std::strcmp(arg, "round")) a.spmv.compact = 1;
        else if (!std::strcmp(arg, "exact")) a.spmv.compact = 2;
        else if (!std::strcmp(arg, "f64")) a.spmv.compact = 3;
        else if (!std::strcmp(arg, "f32")) a.spmv.compact = 4;
        else argp_error(state, "compact: expected 'round' (the default) or 'exact', or 'f64', or 'f32'");
        break;
    case key_alpha:
    case key_beta: {
        char * end = nullptr;
        errno = 0;
        double const value = std::strtod(arg, &end);
        if (errno != 0 || end == arg || *end != '\0')
            argp_error(state, key == key_alpha ? "alpha: expected a number" : "beta: expected a number");
        (key == key_alpha ? a.spmv.alpha : a.spmv.beta) = value;
        a.spmv.scaled = true;
        break;
    }
    case key_dots:
        a.spmv.dots = true;
        break;
    case ARGP_KEY_END:
        if (a.list_perf_events)
            break;
        if (a.spmv.dots && (!a.spmv.scaled || (!a.spmv.f32_values && !a.spmv.compact)))
            argp_error(state, "--dots needs --alpha / --beta and --f32-values or --compact[=f64|f32]: the dots are those of the scaled "
                              "multiplies over float tiles (spmv_hip_run_scaled_dots)");
        if (a.spmv.scaled && !a.spmv.f32_values && !a.spmv.compact)
            argp_error(state, "--alpha / --beta need --f32-values or --compact[=f64|f32]: only the multiplies over float tiles have a scaled "
                              "form, y <- alpha A x + beta y (spmv_hip_run_scaled)");
        if (a.spmv.compact) {
            // what --compact runs on: hip-csr on one device (include/spmv_hip_compact.h); anything else is refused here rather
            // than multiplied some other way
            if (a.spmv.symmetric)
                argp_error(state, "--compact cannot be combined with --symmetric: there is no symmetric kernel over 16-bit column codes");
            if (a.spmv.transpose)
                argp_error(state, "--compact cannot be combined with --transpose: there is no transposed kernel over 16-bit column codes");
            if (a.spmv.vectors > 0)
                argp_error(state, "--compact cannot be combined with --vectors: there is no multi-vector kernel over 16-bit column codes");
            if (a.spmv.f32_values)
                argp_error(state, a.spmv.compact == 3
                               ? "--compact=f64 cannot be combined with --f32-values: it multiplies the fp64 values as they are "
                                 "(--compact stores them as floats)"
                               : "--compact cannot be combined with --f32-values: --compact stores the values as floats already "
                                 "(--compact=exact refuses values that are not floats)");
            if (a.kernel_type != KernelType::spmv || a.format != SpmvFormat::csr)
                argp_error(state, "--compact needs the CSR kernel on the GPU (--spmv-format hip-csr or --csr PATH): "
                                  "there is no COO, ELLPACK or hybrid kernel over 16-bit column codes");
            if (!a.hip && (!a.shortcut || a.device_given))
                argp_error(state, "--compact runs on the GPU only (--spmv-format hip-csr or --device hip): there is no CPU kernel over 16-bit column codes");
            if (a.spmv.num_gpus > 1)
                argp_error(state, "--compact runs on one device (--gpus must be 1)");
        }
        if (a.spmv.f32_values) {
            // what --f32-values runs on: hip-csr on one device (include/spmv_hip_f32values.h); anything else is refused here rather
            // than multiplied some other way
            if (a.spmv.symmetric)
                argp_error(state, "--f32-values cannot be combined with --symmetric: there is no symmetric kernel over float values");
            if (a.spmv.transpose)
                argp_error(state, "--f32-values cannot be combined with --transpose: there is no transposed kernel over float values");
            if (a.spmv.vectors > 0)
                argp_error(state, "--f32-values cannot be combined with --vectors: there is no multi-vector kernel over float values");
            if (a.kernel_type != KernelType::spmv || a.format != SpmvFormat::csr)
                argp_error(state, "--f32-values needs the CSR kernel on the GPU (--spmv-format hip-csr or --csr PATH): "
                                  "there is no COO, ELLPACK or hybrid kernel over float values");
            if (!a.hip && (!a.shortcut || a.device_given))
                argp_error(state, "--f32-values runs on the GPU only (--spmv-format hip-csr or --device hip): there is no CPU kernel over float values");
            if (a.spmv.num_gpus > 1)
                argp_error(state, "--f32-values runs on one device (--gpus must be 1)");
        }
        if (a.spmv.transpose) {
            // what --transpose runs on: hip-csr on one device (include/spmv_hip_transpose.h); anything else is refused here
            // rather than multiplied some other way
            if (a.spmv.symmetric)
                argp_error(state, "--transpose cannot be combined with --symmetric: the matrix a stored triangle stands for is its own transpose");
            if (a.spmv.vectors > 0)
                argp_error(state, "--transpose cannot be combined with --vectors: there is no multi-vector transposed kernel");
            if (a.kernel_type != KernelType::spmv || a.format != SpmvFormat::csr)
                argp_error(state, "--transpose needs the CSR kernel on the GPU (--spmv-format hip-csr or --csr PATH): "
                                  "there is no transposed COO, ELLPACK or hybrid kernel");
            if (!a.hip && (!a.shortcut || a.device_given))
                argp_error(state, "--transpose runs on the GPU only (--spmv-format hip-csr or --device hip): there is no CPU transposed kernel");
            if (a.spmv.num_gpus > 1)
                argp_error(state, "--transpose runs on one device: a row partition would need a reduction of y across devices (--gpus must be 1)");
        }
        if (a.spmv.vectors > 0) {
            // what --vectors runs on: hip-csr on one device (include/spmv_hip_multivec.h); anything else is refused here
            if (a.spmv.symmetric)
                argp_error(state, "--vectors cannot be combined with --symmetric: there is no multi-vector symmetric kernel");
            if (a.kernel_type != KernelType::spmv || a.format != SpmvFormat::csr)
                argp_error(state, "--vectors needs the CSR kernel on the GPU (--spmv-format hip-csr or --csr PATH): "
                                  "there is no multi-vector COO, ELLPACK or hybrid kernel");
            if (!a.hip && (!a.shortcut || a.device_given))
                argp_error(state, "--vectors runs on the GPU only (--spmv-format hip-csr or --device hip): there is no CPU multi-vector kernel");
            if (a.spmv.num_gpus > 1)
                argp_error(state, "--vectors runs on one device (--gpus must be 1)");
        }
        if (a.spmv.symmetric) {
            // what --symmetric runs on: the stored triangle of a (skew-)symmetric matrix, hip-csr on one device; anything else is
            // refused here rather than multiplied some other way
            if (a.spmv.expand_symmetric)
                argp_error(state, "--symmetric multiplies the stored triangle as the whole matrix: it cannot be combined with --expand-symmetric");
            if (a.kernel_type != KernelType::spmv || a.format != SpmvFormat::csr)
                argp_error(state, "--symmetric needs the CSR kernel on the GPU (--spmv-format hip-csr or --csr PATH): "
                                  "there is no symmetric COO, ELLPACK or hybrid kernel");
            if (!a.hip && (!a.shortcut || a.device_given))
                argp_error(state, "--symmetric runs on the GPU only (--spmv-format hip-csr or --device hip): there is no CPU symmetric kernel");
            if (a.spmv.num_gpus > 1)
                argp_error(state, "--symmetric runs on one device: a row partition would send transposed products across devices (--gpus must be 1)");
            if (synthetic::is_spec(a.matrix_path)) {
                if (!synthetic::is_stored_triangle(a.matrix_path))
                    argp_error(state, "--symmetric needs a stored triangle: a synthetic spec ending in :tril, or a file with a "
                                      "`symmetric` or `skew-symmetric` header");
            } else if (!a.matrix_path.empty()) {
                std::string const w = matrix_market::banner_symmetry(a.matrix_path);
                if (w == "general" || w == "hermitian")
                    argp_error(state, "--symmetric needs a file with a `symmetric` or `skew-symmetric` header; %s is %s",
                               a.matrix_path.c_str(), w.c_str());
            }
        }
        if (a.trace_config.empty() && a.threads == 0 && a.write_mtx.empty())
            argp_error(state, "Please specify --trace-config");
        break;
    default: return ARGP_ERR_UNKNOWN;
    }
    return 0;
}

// max_i |y_i - z_i| / max_i |z_i|
// A NaN or an infinity anywhere, or vectors of different lengths, give NaN (which fails the gate).
double relative_error(std::vector<double> const & y, std::vector<double> const & z)
{
    if (y.size() != z.size())
        return std::nan("");
    double err = 0.0, scale = 0.0;
    for (std::size_t i = 0; i < y.size(); ++i) {
        double const d = std::fabs(y[i] - z[i]);
        if (!(d <= err)) // also true when d is NaN
            err = d;
        double const a = std::fabs(z[i]);
        if (!(a <= scale))
            scale = a;
    }
    if (!std::isfinite(err) || !std::isfinite(scale))
        return std::nan("");
    return scale > 0.0 ? err / scale : err;
}

// The exactly rounded sum of finite doubles (Shewchuk's growing expansion of non-overlapping partials): what --dots --check
// restates the device's dots against.  Anything non-finite gives the plain sum.
double exact_sum(std::vector<double> const & t)
{
    std::vector<double> partials;
    for (double x : t) {
        if (!std::isfinite(x)) {
            double plain = 0.0;
            for (double const e : t)
                plain += e;
            return plain;
        }
        std::size_t kept = 0;
        for (double y : partials) {
            if (std::fabs(x) < std::fabs(y))
                std::swap(x, y);
            volatile double const hi = x + y;
            volatile double const back = hi - x;
            double const lo = y - back;
            if (lo != 0.0)
                partials[kept++] = lo;
            x = hi;
        }
        partials.resize(kept);
        partials.push_back(x);
    }
    // the partials do not overlap and grow in magnitude: adding them from the largest down rounds once where the rest is below
    // half an ulp, which holds for all but a tie; the tie is within one ulp of a sum whose bound is rows times wider
    double sum = 0.0;
    for (std::size_t k = partials.size(); k-- > 0;)
        sum += partials[k];
    return sum;
}

// x_i = uniform(-1, 1) from a hash of i: a check with x = 1 only compares row sums
std::vector<double> uniform_x(std::size_t n)
{
    std::vector<double> x(n);
    for (std::size_t i = 0; i < n; ++i) {
        std::uint64_t z = (std::uint64_t) i + 0x9E3779B97F4A7C15ull;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        z ^= z >> 31;
        x[i] = (double) (z >> 11) * (2.0 / 9007199254740992.0) - 1.0;
    }
    return x;
}

} // namespace

int main(int argc, char ** argv)
{
    setlocale(LC_ALL, "");

    argp_option options[] = {
        {"matrix", key_matrix, "PATH", 0, "Read matrix from file in Matrix Market format.", 0},
        {"trace-config", key_trace_config, "PATH", 0,
         "Read cache parameters and thread affinities from a configuration file in JSON format.", 0},
        {"threads", key_threads, "T", 0, "Use a generated configuration with T threads instead of --trace-config (0: the cores this process may use -- affinity mask capped by the cgroup quota)", 0},
        {"profile", key_profile, "N", 0, "Time N runs of the kernel", 0},
        {"warmup", key_warmup, nullptr, 0, "Accepted for compatibility (profiling always warms up once)", 0},
        {"flush-caches", key_flush_caches, nullptr, 0, "Flush CPU caches between each profiling run (hip-* kernels: the device's L2 and Infinity Cache as well)", 0},
        {"list-perf-events", key_list_perf_events, nullptr, 0, "Not available (libpfm4 is not part of this build)", 0},
        {"verbose", key_verbose, nullptr, 0, "be more verbose", 0},
        {"write-mtx", key_write_mtx, "PATH", 0,
         "Write the matrix (--matrix / --synthetic / --csr ...) to PATH as a Matrix Market file (.gz: compressed) that reads "
         "back bit for bit, and stop: files of the generated stand-ins, or a file re-written in plain form", 2},
        {"check", key_check, nullptr, 0,
         "After profiling, compare y with the CPU CSR kernel run the same number of times; adds \"parity\"", 0},

        {nullptr, 0, nullptr, 0, "STREAM-like kernels:", 1},
        {"triad", key_triad, "N", 0, "Triad: a(i)=b(i)+q*c(i), 24 bytes and 2 flops per iteration", 1},

        {nullptr, 0, nullptr, 0, "Sparse matrix-vector multplication kernels:", 2},
        {"spmv-format", key_spmv_format, "FMT", 0,
         "choose one of: coo, coo-atomic, csr, ell, hybrid (CPU, OpenMP) or hip-csr, hip-coo, hip-ell, hip-hybrid (MI355X)", 2},
        {"csr", key_csr, "PATH", 0, "CSR SpMV of the matrix in PATH: on the MI355X when a HIP device is usable (= --spmv-format hip-csr), else "
                                    "the OpenMP kernel with a note on stderr (= --spmv-format csr); --device cpu|hip decides", 2},
        {"coo", key_coo, "PATH", 0, "the same for COO", 2},
        {"ell", key_ell, "PATH", 0, "the same for ELLPACK", 2},
        {"synthetic", key_synthetic, "SPEC", 0,
         "EXTENSION: generate the matrix instead of reading it: poisson2d:<n>, queen[:gx,gy,gz], kkt[:<n>], "
         "webbase[:N,Z,maxrow,locality%], powerlaw[:N,Z,maxrow], banded:N,b[,seed], random:N,k[,seed] (same as --matrix synthetic:SPEC)", 2},
        {"x", key_x, "ones|uniform", 0,
         "EXTENSION: the vector multiplied: all ones like the reference (default), or uniform(-1,1) hashes", 2},
        {"expand-symmetric", key_expand_symmetric, nullptr, 0,
         "EXTENSION: mirror the entries of symmetric files (the reference multiplies the stored triangle only)", 2},
        {"symmetric", key_symmetric, nullptr, 0,
         "EXTENSION (hip-csr, one device): multiply the stored triangle of a symmetric or skew-symmetric file (or a synthetic:...:tril "
         "spec) as the whole matrix -- y += (T + T' - diag T) x, or (T - T') x -- reading every stored value once; --check then "
         "compares with the CPU CSR kernel on the expanded matrix.  Partial sums meet in atomics: not bit-reproducible", 2},
        {"transpose", key_transpose, nullptr, 0,
         "EXTENSION (hip-csr, one device): y += A' x from the arrays of A as they are stored (x has rows entries, y has columns); "
         "no transposed copy is made.  --check compares with the CPU CSR kernel on the matrix transposed on the host", 2},
        {"f32-values", key_f32_values, "round|exact", OPTION_ARG_OPTIONAL,
         "EXTENSION (hip-csr, one device): store and stream the matrix values as 4-byte floats, every product and sum in fp64 "
         "(8 instead of 12 bytes per stored entry).  round (default): values are rounded to the nearest float and the JSON "
         "document says how many and by how much; exact: a matrix with values that are not floats already is refused.  --check "
         "compares with the CPU CSR kernel on the values rounded on the host", 2},
        {"compact", key_compact, "round|exact|f64|f32", OPTION_ARG_OPTIONAL,
         "EXTENSION (hip-csr, one device): --f32-values with the columns of a tile streamed as 16-bit codes, a 3-bit window number "
         "and a 13-bit offset from one of eight per-tile bases (6 instead of 8 bytes per stored entry); tiles that need more "
         "than eight windows keep their 32-bit columns, and the JSON document counts both kinds.  round (default) and exact are "
         "those of --f32-values.  --check compares with the CPU CSR kernel on the values rounded on the host.  f64: the same "
         "16-bit codes beside the fp64 values as they are (10 instead of 12 bytes per stored entry, nothing is rounded: "
         "kernel hip-csr-spmv-compact-f64); --check compares with the CPU CSR kernel on the unrounded values.  f32: round with x "
         "and y stored as 4-byte floats on the device as well, every row's fp64 sum rounded to float once per run (kernel "
         "hip-csr-spmv-compact-f32); --check compares with the CPU CSR kernel on the values and x rounded to float on the host, "
         "with a tolerance that grows with the number of runs", 2},
        {"alpha", key_alpha, "A", 0,
         "EXTENSION (with --f32-values or --compact[=f64|f32]): every run is y <- A * (matrix x) + B * y instead of y += matrix x, in "
         "one launch (spmv_hip_run_scaled); A and B default to 1, and the JSON document names both.  --check compares with the CPU "
         "CSR kernel's product put through the same number of scaled steps on the host", 2},
        {"beta", key_beta, "B", 0, "EXTENSION: see --alpha", 2},
        {"dots", key_dots, 0, 0,
         "EXTENSION (with --alpha / --beta): every run also computes y' y and x' y of the y it has just written, in the same launch "
         "(spmv_hip_run_scaled_dots; x' y only where the matrix is square, otherwise 0); the JSON document names those of the last run "
         "as \"dots\".  --check restates both on the host from the y it reads back, within rows 2^-53 sum |products|", 2},
        {"vectors", key_vectors, "K", 0,
         "EXTENSION (hip-csr, one device): Y += A X for K = 1 ... 16 vectors in one multiply, every stored entry read once; column c "
         "of X is x scaled by c + 1.  Flops count 2 nnz K; --check compares every column with the CPU CSR kernel", 2},
        {"matrix-cache", key_matrix_cache, "DIR", 0,
         "EXTENSION: keep the parsed entries of every matrix file in DIR and read them back next time "
         "(keyed by path, size and modification time; also: environment SPMV_MATRIX_CACHE)", 2},

        {nullptr, 0, nullptr, 0, "GPU:", 3},
        {"device", key_device, "cpu|hip", 0,
         "Where the kernel runs: cpu (the reference's OpenMP kernels) or hip (MI355X; an error without a usable device). Default: "
         "--csr/--coo/--ell PATH pick hip when a device is usable, --spmv-format FMT and --triad mean what they name; the "
         "environment variable SPMV_DEVICE=cpu|hip sets the default of them all", 3},
        {"gpu", key_gpu, "INDEX", 0, "HIP device index (default 0)", 3},
        {"gpus", key_gpus, "G", 0,
         "hip-csr, hip-coo, hip-ell: partition the rows over devices 0..G-1 (the reference's static chunks, ceil(rows/G) rows each), "
         "x replicated, one RCCL all-gather of y per run", 3},
        {"pipeline-gather", key_pipeline_gather, nullptr, 0,
         "hip-* kernels with --gpus G > 1 (RCCL or --peer-gather): back-to-back runs overlap -- the gather of run k travels on a second "
         "stream per device while run k + 1 multiplies (two alternating copies of y).  The timed loop of --profile waits for every "
         "run, so its samples do not change; callers that enqueue several runs before they wait get max(multiply, gather) per run", 6},
        {"balance-entries", key_balance_entries, nullptr, 0,
         "with --gpus: cut the rows at equal shares of the stored entries instead of ceil(rows/G) rows per device", 3},
        {"peer-gather", key_peer_gather, nullptr, 0,
         "with --gpus: gather y by remote stores over xGMI (one kernel per device) instead of RCCL", 3},
        {"fused-peer-store", key_fused_peer_store, nullptr, 0,
         "with --gpus: every device's multiply stores its row sums into all devices' y itself (no RCCL, no gather launch)", 3},
        {"csr-algorithm", key_csr_algorithm, "NAME", 0, "auto, scalar, vector, adaptive or wavetile", 3},
        {"lanes-per-row", key_lanes, "L", 0, "lanes per row of the vector algorithm (2..64, power of two)", 3},
        {"exact-order", key_exact_order, nullptr, 0, "sum every row left to right like the CPU loop (bit-exact)", 3},
        {nullptr, 0, nullptr, 0, nullptr, 0}};

    argp parser{options, parse_option, nullptr,
                "Time sparse matrix-vector multiplication (y += A*x) on CPU threads or on an MI355X",
                nullptr, nullptr, nullptr};

    Arguments args;
    if (error_t err = argp_parse(&parser, argc, argv, 0, nullptr, &args)) {
        std::cerr << strerror(err) << '\n';
        return err;
    }

    if (args.list_perf_events) {
        std::cerr << "Please re-build with libpfm enabled\n"; // the reference's NO_LIBPFM message
        return EXIT_FAILURE;
    }
    if (!args.write_mtx.empty()) {
        if (args.matrix_path.empty()) {
            std::cerr << "--write-mtx needs a matrix (--matrix PATH, --synthetic SPEC or --csr/--coo/--ell PATH)\n";
            return EXIT_FAILURE;
        }
        try {
            matrix_market::Matrix m = matrix_market::load_matrix(args.matrix_path, std::cerr, args.verbose);
            if (args.spmv.expand_symmetric)
                m = matrix_market::expand_symmetry(m);
            matrix_market::write_matrix(args.write_mtx, m);
            std::cout << "{\"written\": \"" << args.write_mtx << "\", \"rows\": " << m.rows() << ", \"columns\": " << m.columns()
                      << ", \"entries\": " << m.num_entries() << "}\n";
            return EXIT_SUCCESS;
        } catch (std::exception const & e) {
            std::cerr << e.what() << "\n";
            return EXIT_FAILURE;
        }
    }

    if (args.kernel_type == KernelType::none) {
        std::cerr << "Please choose a kernel: --spmv-format FMT --matrix PATH, --csr/--coo/--ell PATH or --triad N\n";
        return EXIT_FAILURE;
    }

    // runtime switch for drop-in use: SPMV_DEVICE=hip makes the GPU the default of every format
    // option that does not say otherwise (an explicit --device / hip-* always wins); anything but
    // "hip" or "cpu" is an error, and a GPU default without a usable GPU fails like --device hip
    bool env_decides = false;
    if (char const * env = std::getenv("SPMV_DEVICE")) {
        if (!std::strcmp(env, "hip") || !std::strcmp(env, "gpu")) {
            if (!args.device_given)
                args.hip = true;
            env_decides = true;
        } else if (!std::strcmp(env, "cpu")) {
            env_decides = true;
        } else if (*env) {
            std::cerr << "SPMV_DEVICE: expected 'cpu' or 'hip'\n";
            return EXIT_FAILURE;
        }
    }
    // --csr / --coo / --ell PATH, the README's spelling (README.md:81,124), is what a user of the reference types: as the drop-in
    // for that path it runs the MI355X kernel whenever a device is usable and nothing said otherwise (--device, SPMV_DEVICE, an
    // explicit --spmv-format); without one it runs the reference's OpenMP kernel and says so in one line -- never silently.
    if (args.shortcut && !args.device_given && !env_decides && args.kernel_type == KernelType::spmv) {
        int count = 0;
        if (spmv_hip_device_count(&count) == 0 && count > 0)
            args.hip = true;
        else if (!args.spmv.symmetric && args.spmv.vectors == 0 && !args.spmv.transpose && !args.spmv.f32_values && !args.spmv.compact) // (those fail below: nothing runs in their place)
            std::cerr << "note: no usable HIP device: the CPU (OpenMP) kernel runs (--device hip makes this an error, --device cpu silences the note)\n";
    }

    if (args.spmv.symmetric && !args.hip) {
        std::cerr << "--symmetric: the kernel would run on the CPU (no usable HIP device, or SPMV_DEVICE=cpu), and there is no CPU symmetric kernel "
                     "(nothing runs in its place)\n";
        return EXIT_FAILURE;
    }

    if (args.spmv.transpose && !args.hip) {
        std::cerr << "--transpose: the kernel would run on the CPU (no usable HIP device, or SPMV_DEVICE=cpu), and there is no CPU transposed "
                     "kernel (nothing runs in its place)\n";
        return EXIT_FAILURE;
    }

    if (args.spmv.f32_values && !args.hip) {
        std::cerr << "--f32-values: the kernel would run on the CPU (no usable HIP device, or SPMV_DEVICE=cpu), and there is no CPU kernel over "
                     "float values (nothing runs in its place)\n";
        return EXIT_FAILURE;
    }

    if (args.spmv.compact && !args.hip) {
        std::cerr << "--compact: the kernel would run on the CPU (no usable HIP device, or SPMV_DEVICE=cpu), and there is no CPU kernel over "
                     "16-bit column codes (nothing runs in its place)\n";
        return EXIT_FAILURE;
    }

    if (args.spmv.vectors > 0 && !args.hip) {
        std::cerr << "--vectors: the kernel would run on the CPU (no usable HIP device, or SPMV_DEVICE=cpu), and there is no CPU multi-vector "
                     "kernel (nothing runs in its place)\n";
        return EXIT_FAILURE;
    }

    std::unique_ptr<Kernel> kernel;
    if (args.kernel_type == KernelType::triad)
        kernel = make_triad_kernel(args.triad_entries, args.hip, args.spmv.device);
    else
        kernel = make_spmv_kernel(args.format, args.hip, args.matrix_path, args.spmv);

    try {
        TraceConfig trace_config =
            args.trace_config.empty() ? default_trace_config(args.threads) : read_trace_config(args.trace_config);

        if (args.profile == 0) {
            std::cerr << "Cache tracing (the mode without --profile) is not part of this engine: "
                         "use --profile=N to time the kernel\n";
            return EXIT_FAILURE;
        }

        kernel->init(trace_config, std::cerr, args.verbose);
        std::vector<double> xv;
        if (args.x_uniform && args.kernel_type == KernelType::spmv) {
            xv = uniform_x(kernel->columns());
            kernel->set_x(xv);
        }
        Profiling profiling =
            profile_kernel(trace_config, *kernel, true, args.flush_caches, args.profile, std::cerr, args.verbose);

        std::string parity;
        bool const workspace_recurrence = !args.hip && (args.format == SpmvFormat::coo || args.format == SpmvFormat::hybrid)
            && trace_config.thread_affinities().size() > 1;
        if (args.check && args.kernel_type == KernelType::spmv && workspace_recurrence) {
            // the reference's multi-threaded COO kernel scatters into per-thread workspaces that are never cleared
            // (src/matrix/coo-matrix.cpp:248-285, src/kernels/coo-spmv.cpp:41-48): run k adds k * A x, so y after the
            // timed loop is not (runs) * A x and there is nothing to compare with -- reproduced faithfully, hence no verdict
            parity = ",\n\"parity\": {\"against\": \"csr-spmv (CPU, 1 thread)\", \"skipped\": \"the CPU COO kernel on more than one thread "
                     "accumulates its workspace across runs like the reference's (coo-matrix.cpp:248-285); use --threads 1 or a hip-* kernel\", "
                     "\"pass\": null}";
        } else if (args.check && args.kernel_type == KernelType::spmv) {
            // the same matrix through the CPU CSR kernel, one thread, warm-up + N accumulating runs
            TraceConfig one = default_trace_config(1);
            // (--symmetric: the matrix expand_symmetry builds from the same file -- an independent path to the same product)
            SpmvOptions ref_options = args.spmv;
            if (args.spmv.symmetric) {
                ref_options.symmetric = false;
                ref_options.expand_symmetric = true;
            }
            // (--transpose: the matrix transposed on the host by a stable counting sort -- again an independent path)
            if (args.spmv.transpose) {
                ref_options.transpose = false;
                ref_options.transpose_on_host = true;
            }
            // (--f32-values: the values rounded on the host by static_cast<float> -- an independent path to the same operator)
            bool const rounded = args.spmv.f32_values || args.spmv.compact == 1 || args.spmv.compact == 2 || args.spmv.compact == 4; // (--compact=f64 rounds nothing)
            bool const float_vectors = args.spmv.compact == 4; // (--compact=f32: x is rounded too, and y once per row and run)
            ref_options.compact = 0;
            if (rounded) {
                ref_options.f32_values = 0;
                ref_options.compact = 0;
                ref_options.round_values_on_host = true;
            }
            ref_options.vectors = 0;
            ref_options.scaled = false; // (--alpha / --beta: the CPU kernel multiplies once, and the scaled steps are restated below)
            double err = 0.0;
            int const k = std::max(1, args.spmv.vectors);
            std::vector<double> const got = kernel->result();
            // --vectors: column c of Y against the CPU kernel with x scaled by c + 1, the worst column counts
            for (int c = 0; c < k; ++c) {
                std::unique_ptr<Kernel> ref = make_spmv_kernel(SpmvFormat::csr, false, args.matrix_path, ref_options);
                ref->init(one, std::cerr, false);
                if (!xv.empty() || args.spmv.vectors > 0) {
                    std::vector<double> xc = xv.empty() ? std::vector<double>(ref->columns(), 1.0) : xv;
                    for (double & e : xc)
                        e *= c + 1.0;
                    if (float_vectors)
                        for (double & e : xc)
                            e = static_cast<double>(static_cast<float>(e));
                    ref->set_x(xc);
                }
                for (int r = 0; r < (args.spmv.scaled ? 1 : args.profile + 1); ++r)
                    ref->run(one);
                std::vector<double> want = ref->result();
                if (args.spmv.scaled) {
                    // y <- alpha z + beta y from y = 0, run by run, with z = A x from the CPU kernel: two products and a sum, each
                    // rounded; --compact=f32 rounds y to float once per run
                    std::vector<double> const z = want;
                    std::fill(want.begin(), want.end(), 0.0);
                    for (int r = 0; r < args.profile + 1; ++r)
                        for (std::size_t i = 0; i < want.size(); ++i) {
                            volatile double const az = args.spmv.alpha * z[i], by = args.spmv.beta * want[i];
                            double const yi = args.spmv.alpha == 0.0 ? by : (args.spmv.beta == 0.0 ? az : az + by);
                            want[i] = float_vectors ? static_cast<double>(static_cast<float>(yi)) : yi;
                        }
                }
                std::vector<double> col = got;
                if (args.spmv.vectors > 0) {
                    col.assign(got.size() / (std::size_t) k, 0.0);
                    for (std::size_t i = 0; i < col.size(); ++i)
                        col[i] = got[i * (std::size_t) k + (std::size_t) c];
                }
                double const e = relative_error(col, want);
                if (!(e <= err)) // NaN sticks
                    err = e;
            }
            parity = ",\n\"parity\": {\"against\": \"csr-spmv (CPU, 1 thread)" +
                std::string(args.spmv.symmetric ? " on the expanded matrix (expand_symmetry)" : "") +
                std::string(args.spmv.transpose ? " on the matrix transposed on the host" : "") +
                std::string(rounded ? (float_vectors ? " on the values and x rounded to float on the host" : " on the values rounded to float on the host") : "") +
                (args.spmv.vectors > 0 ? ", every one of the " + std::to_string(k) + " columns" : std::string()) + ", " +
                std::to_string(args.profile + 1) + (args.spmv.scaled ? " scaled runs (y <- alpha A x + beta y) restated on the host" : " accumulating runs") +
                "\", \"max_relative_error\": ";
            char buf[64];
            if (std::isnan(err))
                std::snprintf(buf, sizeof buf, "\"nan\"");
            else
                std::snprintf(buf, sizeof buf, "%.3e", err);
            parity += buf;
            bool dots_pass = true;
            std::string dots_report;
            double device_dots[2];
            if (kernel->last_dots(device_dots)) {
                // --dots: both restated from the y read back, t_i the rounded products and their exactly rounded sum; any order of
                // adding them in fp64 stays within rows 2^-53 sum |t_i| of it.  x is what the device holds (all ones, or --x uniform; floats
                // under --compact=f32), and only a square matrix has an x' y
                std::size_t const n = got.size();
                bool const square = n == kernel->columns();
                std::vector<double> t[2] = {std::vector<double>(n), std::vector<double>(n, 0.0)};
                for (std::size_t i = 0; i < n; ++i) {
                    double xi = xv.empty() ? 1.0 : (i < xv.size() ? xv[i] : 0.0);
                    if (float_vectors)
                        xi = static_cast<double>(static_cast<float>(xi));
                    volatile double const yy = got[i] * got[i], xy = square ? xi * got[i] : 0.0;
                    t[0][i] = yy;
                    t[1][i] = xy;
                }
                dots_report = ", \"dots\": {\"restated\": [";
                std::string bounds;
                for (int d = 0; d < 2; ++d) {
                    double const want = exact_sum(t[d]);
                    double mag = 0.0;
                    for (double const e : t[d])
                        mag += std::fabs(e);
                    double const bound = (double) n * std::ldexp(1.0, -53) * mag;
                    if (!(std::fabs(device_dots[d] - want) <= bound)) // (false for NaN)
                        dots_pass = false;
                    std::snprintf(buf, sizeof buf, std::isfinite(want) ? "%.17g" : "\"%g\"", want);
                    dots_report += std::string(buf) + (d == 0 ? ", " : "]");
                    std::snprintf(buf, sizeof buf, std::isfinite(bound) ? "%.3e" : "\"%g\"", bound);
                    bounds += std::string(buf) + (d == 0 ? ", " : "]");
                }
                dots_report += ", \"bound\": [" + bounds + ", \"pass\": " + (dots_pass ? "true" : "false") + "}";
            }
            // --compact=f32: run k rounds a y of magnitude about k s once, so after R runs the roundings sum to at most
            // 2^-24 s R (R + 1) / 2 against a result of R s: (R + 1) 2^-25, and the fp64 additions' share in the factor beside it
            double tolerance = 1e-10;
            if (float_vectors)
                tolerance += (args.profile + 2.0) * std::ldexp(1.0, -25) * (1.0 + std::ldexp(1.0, -10));
            std::snprintf(buf, sizeof buf, "%.6e", tolerance);
            // err <= tolerance is false for NaN: non-finite values and size mismatches fail
            parity += std::string(", \"tolerance\": ") + (float_vectors ? buf : "1e-10") + ", \"pass\": " + (err <= tolerance ? "true" : "false") + dots_report + "}";
        }

        profiling.set_extra(parity);
        {
            json_ostreambuf pretty(std::cout);
            std::cout << profiling << '\n';
        }
        if (!parity.empty() && parity.find("\"pass\": false") != std::string::npos) {
            std::cerr << kernel->name() << ": parity check failed\n";
            return EXIT_FAILURE;
        }
    } catch (trace_config_error const & e) {
        std::cerr << args.trace_config << ": " << e.what() << '\n';
        return EXIT_FAILURE;
    } catch (kernel_error const & e) {
        std::cerr << kernel->name() << ": " << e.what() << '\n';
        return EXIT_FAILURE;
    } catch (std::system_error const & e) {
        std::cerr << e.what() << '\n';
        return EXIT_FAILURE;
    }
    return EXIT_SUCCESS;
}
