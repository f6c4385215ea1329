// The power-flow plan (include/csparse3_amd.h, "AC power flow"): what powerflow.cpp builds on the host and powerflow.hip
// uploads, reads and drives.  Host code only.
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/csparse3_amd.h"
#include "cs3_hipmem.hpp"

namespace cs3 {

constexpr int PF_BLOCK = 256;
constexpr int PF_GRID_CAP = 1024;          // workgroups per scenario; beyond PF_GRID_CAP * PF_BLOCK items a lane loops
constexpr int PF_WAVE_ROW = 64;            // a row of Y with more stored entries than this is summed by a whole wave

}  // namespace cs3

struct cs3_pf_s {
    int64_t n = 0, nnz_y = 0, npv = 0, npq = 0, nref = 0, nj = 0, nnz_j = 0, batch = 1, y_batch = 1;
    int64_t rows_lane = 0, rows_wave = 0, max_row = 0;
    std::vector<int32_t> Jp, Ji;            // the Jacobian's pattern [[H, N], [M, L]]
    std::vector<int32_t> jpos;              // [4][nnz_y]: where entry q of Y lands in H, N, M, L; -1: nowhere
    std::vector<int32_t> yrow, ycol;        // [nnz_y] row and column of every stored entry
    std::vector<int32_t> Rp, Rj, Rpos;      // Y by rows: ascending column, and the entry of Yz behind every one
    std::vector<int32_t> upos_a, upos_m;    // [n] the unknown behind theta_i / |V|_i, -1: none (upos_m counts from npv + npq)
    std::vector<int32_t> ubus;              // [nj] the bus behind every unknown (pv ++ pq ++ pq)
    std::vector<int32_t> wave_rows;         // the non-reference rows longer than PF_WAVE_ROW, ascending
    cs3_handle h = nullptr;                 // the batched LU handle on (Jp, Ji): owned here, lent by cs3_pf_handle
    // device copies of the tables (cs3_pf_upload) and the driver's work arrays
    bool uploaded = false;
    struct Memory {
        cs3::DevBuf<int32_t> jpos, yrow, ycol, Rp, Rj, Rpos, upos_a, upos_m, ubus, wave_rows;
        cs3::DevBuf<double> rhs, cur, jx, norm;            // [batch][nj], [batch][n][2], [batch][nnz_j], [batch]
        cs3::DevBuf<unsigned long long> nbits;             // [batch] bit pattern of the running max |F|
        cs3::DevBuf<int32_t> ints;                         // state [batch], iters [batch], flag [batch], active [1]
    } mem;
};

// What powerflow.cpp (the plan, the driver) calls of powerflow.hip (the tables on the device, the launches).  Every
// pointer is a device address; `state` [batch] may be null (every scenario active).
namespace cs3 {

int pf_upload(cs3_pf_s *p);
// -F into rhs [batch][nj] (S null: currents only), I into the plan's current buffer, max |F| into nbits by integer max
int pf_launch_mismatch(cs3_pf_s *p, const double *Yz, const double *S, const double *vm, const double *va, const int32_t *state,
                       double *rhs, unsigned long long *nbits, hipStream_t st);
int pf_launch_jacobian(cs3_pf_s *p, const double *Yz, const double *vm, const double *va, const int32_t *state, double *Jx,
                       hipStream_t st);
int pf_launch_init(cs3_pf_s *p, hipStream_t st);
int pf_launch_decide(cs3_pf_s *p, int it, int max_iters, double tol, hipStream_t st);
int pf_launch_update(cs3_pf_s *p, double *vm, double *va, const int *status, hipStream_t st);

}  // namespace cs3
