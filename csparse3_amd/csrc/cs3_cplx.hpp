// The complex plan (include/csparse3_amd.h, "complex matrices"): what cplxplan.cpp builds on the host and cplxplan.hip
// uploads and reads.  Host code only.
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/csparse3_amd.h"
#include "cs3_hipmem.hpp"

struct cs3_cplx_s {
    int64_t n = 0, nnz = 0, batch = 1, rotate = 0, rows_without_diagonal = 0;
    std::vector<int32_t> Ap, Ai;            // the complex pattern as given (storage order kept)
    std::vector<int32_t> ecol;              // [nnz] the column of every entry
    std::vector<int32_t> dptr, dpos;        // [n + 1], [.] the stored (i, i) entries of every column, storage order
    std::vector<int32_t> rptr, rpos;        // [n + 1], [nnz] the entries of every row: ascending column, storage order inside
    // a plan with a border (cs3_cplx_plan_create_schur): the rows that are never rotated, in the caller's order; their
    // lists in dptr / dpos are empty
    std::vector<int32_t> schur_idx;
    // device copies (cs3_cplx_upload) and the rotation s [batch][n] complex of the last values call
    bool uploaded = false;
    cs3::DevBuf<int32_t> d_Ap, d_Ai, d_ecol, d_dptr, d_dpos, d_rptr, d_rpos;
    cs3::DevBuf<double> d_s;
    // grow-only blocks for callers that keep nothing of their own (cs3_cplx_workspace_dev)
    cs3::DevBuf<double> ws[3];
};
