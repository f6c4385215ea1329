// The union plan (include/csparse3_amd.h, "union plans"): what unionplan.cpp builds on the host and unionplan.hip uploads
// and reads.  Host code only.
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/csparse3_amd.h"
#include "cs3_hipmem.hpp"

struct cs3_union_s {
    int64_t n = 0, nmat = 0, nnz_u = 0, nnz_total = 0, nmaps = 0, padded = 0, dup_slots = 0;
    std::vector<int32_t> Up, Ui;            // the union pattern, rows ascending
    std::vector<int32_t> map_of;            // [nmat] the distinct pattern of every member
    std::vector<long long> off;              // [nmat + 1] entries before every member in the ragged value buffer
    std::vector<std::vector<int32_t>> slot; // [nmaps][nnz of the pattern] union entry of every member entry
    // the gather map, [nmaps][nnz_u]: >= 0 the one source, -1 none, <= -2 the list -2 - v of ovs[ovp[.] .. ovp[. + 1])
    std::vector<int32_t> map;
    std::vector<long long> ovp;              // [lists + 1]
    std::vector<int32_t> ovs;               // sources of the duplicate slots, storage order inside a list
    // device copies (cs3_union_upload)
    bool uploaded = false;
    cs3::DevBuf<int32_t> d_map, d_map_of, d_ovs;
    cs3::DevBuf<long long> d_off, d_ovp;
};
