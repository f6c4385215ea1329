// The state-estimation plan (include/csparse3_amd.h, "AC state estimation"): what stateest.cpp builds on the host and
// stateest.hip uploads, reads and drives.  Host code only.
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/csparse3_amd.h"
#include "cs3_hipmem.hpp"

namespace cs3 {

constexpr int SE_BLOCK = 256;
constexpr int SE_GRID_CAP = 1024;          // workgroups of the entry kernel; beyond SE_GRID_CAP * SE_BLOCK entries a lane loops
constexpr int SE_WAVE_ROW = 64;            // a row of Y with more stored entries than this is summed by a whole wave
constexpr int SE_WAVE_COL = 64;            // a column of H with more entries than this is summed by a whole wave

// what an entry of H is (e_code): bits 0-1 the family, bit 2 the imaginary part (Q), bit 3 d/d|V| (else d/dtheta),
// bit 4 the near side: the diagonal of an injection row, the from-bus of a flow row
constexpr int SE_E_ONE = 0, SE_E_INJ = 1, SE_E_FLOW = 2;
constexpr int SE_E_IMAG = 4, SE_E_MAG = 8, SE_E_NEAR = 16;

}  // namespace cs3

struct cs3_se_s {
    int64_t n = 0, nnz_y = 0, nref = 0, na = 0, ns = 0, ne = 0, m = 0, nnz_h = 0, order = 1;
    int64_t nkind[5] = {0, 0, 0, 0, 0};
    int64_t max_row = 0, max_col = 0;
    std::vector<int32_t> Rp, Rj, Rpos;      // Y by rows: ascending column, and the entry of Yz behind every one
    std::vector<int32_t> upos_a, upos_m;    // [n] the state behind theta_i (-1: a reference bus) / |V|_i
    std::vector<int32_t> sbus;              // [ns] the bus behind every state
    std::vector<int32_t> kind, where;       // [m]
    std::vector<int32_t> end_from, end_to;  // [ne]
    std::vector<int32_t> Hrp, Hrj;          // H by rows: what cs3_quad_plan takes as Ct
    std::vector<int32_t> Hp, Hi;            // H in CSC, ascending measurement inside a column
    std::vector<int32_t> cpos;              // [nnz_h] row-order entry -> CSC position
    std::vector<int32_t> e_row, e_src, e_code, e_bus;   // [nnz_h] per row-order entry: measurement, entry of Yz or end, SE_E_*, the state's bus
    std::vector<int32_t> wave_rows;         // rows of Y longer than SE_WAVE_ROW, ascending
    std::vector<int32_t> wave_cols;         // columns of H longer than SE_WAVE_COL, ascending
    // built by the first call that needs the solver (se_ensure_solver)
    cs3_spgemm gain = nullptr;              // H' (W H) on H's CSC pattern
    cs3_handle h = nullptr;                 // the Cholesky handle on the gain matrix: owned here, lent by cs3_se_handle
    cs3_quadplan quad = nullptr;            // the rows of H on that handle
    std::vector<int32_t> Gp, Gi;
    // device copies of the tables (se_upload) and the work arrays
    bool uploaded = false, work = false;
    struct Memory {
        cs3::DevBuf<int32_t> Rp, Rj, Rpos, sbus, kind, where, end_from, end_to, Hp, Hi, cpos, e_row, e_src, e_code, e_bus, wave_rows, wave_cols;
        cs3::DevBuf<double> cur;                           // [n][4]: Re I, Im I, cos theta, sin theta
        cs3::DevBuf<double> r, wr, parts, jsum;            // [m], [m], [ceil(m / 256)], [1]
        cs3::DevBuf<unsigned long long> dxbits;            // [1] bit pattern of max |dx|
        cs3::DevBuf<double> hr, hc, whc, gx, rhs;          // [nnz_h] x 3, [nnz_g], [ns]
    } mem;
};

// What stateest.cpp calls of stateest.hip.  Every pointer is a device address.
namespace cs3 {

int se_upload(cs3_se_s *p);
// I and (cos, sin) of every bus into the plan's current buffer; clears the max |dx| word
int se_launch_currents(cs3_se_s *p, const double *Yz, const double *vm, const double *va, hipStream_t st);
// r = z - h(x) into the plan (and r_out when not null), w r into the plan, the partials of sum w r^2; with J_out the closing workgroup
int se_launch_residual(cs3_se_s *p, const double *Ye, const double *z, const double *w, const double *vm, double *r_out, double *J_out,
                       hipStream_t st);
int se_launch_jacobian(cs3_se_s *p, const double *Yz, const double *Ye, const double *w, const double *vm, double *Hr, double *Hc,
                       double *WHc, hipStream_t st);
// g = Hc' wr
int se_launch_gradient(cs3_se_s *p, const double *Hc, const double *wr, double *g, hipStream_t st);
int se_launch_update(cs3_se_s *p, const double *dx, double *vm, double *va, const int *status, hipStream_t st);

}  // namespace cs3
