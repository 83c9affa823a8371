// spmv-kernels.hpp -- the SpMV kernel types behind the Kernel interface.
//
//   csr_spmv_kernel / coo_spmv_kernel / coo_spmv_atomic_kernel / ell_spmv_kernel
//       the reference's CPU kernels (src/kernels/{csr,coo,coo-spmv-atomic,ell}-spmv.cpp):
//       OpenMP loops over host arrays.  They keep the CLI's CPU path (BASELINE configs[0]).
//   hip_csr_spmv_kernel / hip_coo_spmv_kernel / hip_ell_spmv_kernel
//       the same three formats multiplied on an MI355X through the C ABI (include/spmv_hip.h).
//       No fallback: if the device library cannot run, init() throws kernel_error.
//   hip_csr_symmetric_spmv_kernel (--symmetric)
//       the stored triangle of a symmetric / skew-symmetric file multiplied as the whole matrix, each stored value read once.
//   hip_csr_f32values_spmv_kernel (--f32-values)
//       y += fl32(A) x: the values stored and streamed as 4-byte floats, products and sums in fp64 (hip-csr-spmv-f32values).
//   hip_csr_compact_spmv_kernel (--compact)
//       ... with the columns of a tile as 16-bit window codes, 6 bytes per stored entry (hip-csr-spmv-compact).
//       --compact=f32: ... and x and y as 4-byte floats, every row's fp64 sum rounded once per run (hip-csr-spmv-compact-f32).
//   hip_csr_compact_f64_spmv_kernel (--compact=f64)
//       the fp64 values as they are beside the 16-bit window codes, 10 bytes per stored entry (hip-csr-spmv-compact-f64).
//   hip_csr_transposed_spmv_kernel (--transpose)
//       y += A' x from the CSR arrays of A as they are (x has rows entries, y has columns); no transposed copy is made.
//
// All of them load the matrix in init() exactly as the reference does (Matrix Market file ->
// format conversion, x = 1.0, y = 0.0, errors rewrapped as "<path>: <what>") and print the same
// JSON object (name, matrix_path, matrix_format, rows, columns, nonzeros, matrix_size, x_size,
// y_size); the HIP kernels add a "device" object.
#pragma once

#include "kernel.hpp"

#include "../matrix/coo-matrix.hpp"
#include "../matrix/csr-matrix.hpp"
#include "../matrix/ell-matrix.hpp"
#include "../matrix/hybrid-matrix.hpp"

#include <memory>
#include <string>

struct spmv_hip_ctx;

// Options shared by every SpMV kernel type (all default to the reference's behaviour).
struct SpmvOptions
{
    bool expand_symmetric = false; // EXTENSION: mirror symmetric files
    int device = 0;                // HIP device index
    int num_gpus = 0;              // > 0: rows partitioned over devices 0..num_gpus-1 (spmv_hip_create_multi; CSR only)
    int csr_algorithm = 0;         // SPMV_HIP_CSR_*
    int csr_lanes_per_row = 0;
    unsigned hip_flags = 0;        // SPMV_HIP_FLAG_*
    bool symmetric = false;        // EXTENSION: multiply the stored triangle of a (skew-)symmetric file as the whole matrix
                                   // (hip-csr only: spmv_hip_upload_csr_symmetric, include/spmv_hip_symmetric.h)
    bool transpose = false;        // EXTENSION: y += A' x from the arrays of A as stored (hip-csr, one device:
                                   // spmv_hip_upload_csr_transposed, include/spmv_hip_transpose.h)
    int f32_values = 0;            // EXTENSION: 1 = the values are stored and streamed as 4-byte floats, rounded where they must be
                                   // (--f32-values, --f32-values=round); 2 = values that are not floats already are refused
                                   // (--f32-values=exact): hip-csr, one device (spmv_hip_upload_csr_f32values, spmv_hip_f32values.h)
    bool scaled = false;           // EXTENSION: --alpha / --beta were given: every run is y <- alpha A x + beta y (spmv_hip_run_scaled,
    double alpha = 1.0, beta = 1.0; // spmv_hip_scaled.h), with --f32-values or --compact only
    bool dots = false;             // EXTENSION: --dots, with --alpha / --beta: every run also leaves y' y and x' y of the new y on the device
                                   // (spmv_hip_run_scaled_dots, spmv_hip_dots.h)
    int compact = 0;               // EXTENSION: --f32-values (1 = round, 2 = exact) with the columns of a tile as 16-bit window codes
                                   // (--compact[=round|exact]): hip-csr, one device (spmv_hip_upload_csr_compact, spmv_hip_compact.h)
                                   // 3 = f64 (--compact=f64): the fp64 values as they are beside the codes (spmv_hip_upload_csr_compact_f64)
                                   // 4 = f32 (--compact=f32): 1 with x and y as floats on the device (spmv_hip_upload_csr_compact_f32xy)
    bool round_values_on_host = false; // the CPU CSR kernel multiplies the values rounded by static_cast<float>: what --check
                                   // compares --f32-values with (set by the program, not by an option)
    bool transpose_on_host = false; // the CPU CSR kernel multiplies the matrix transposed on the host: what --check compares
                                   // --transpose with (set by the program, not by an option)
    int vectors = 0;               // EXTENSION: > 0: Y += A X for that many vectors (hip-csr, one device: include/spmv_hip_multivec.h)
};

enum class SpmvFormat { csr, coo, coo_atomic, ell, hybrid };

// Factory: `hip` selects the GPU implementation of the format.
std::unique_ptr<Kernel> make_spmv_kernel(SpmvFormat format, bool hip, std::string const & matrix_path,
                                         SpmvOptions const & options = SpmvOptions());
