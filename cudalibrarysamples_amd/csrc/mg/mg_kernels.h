// Device helpers of libcutensorMg.so (mg_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

constexpr int kMgCopyBatch = 16;    // cells per launch: 16 x (source, destination, bytes) = 388 bytes of kernel arguments

struct MgCopyBatch {
    const void* src[kMgCopyBatch];
    void* dst[kMgCopyBatch];
    uint64_t bytes[kMgCopyBatch];
    int n = 0;
};

// dst[i][0 .. bytes[i]) = src[i][0 .. bytes[i]) for i < n, one launch on `stream` of the current device (same-device memory)
hipError_t mg_copy_cells(const MgCopyBatch& batch, hipStream_t stream);

// ---- cutensorMgCopy (mg_redistribute.hip; index arithmetic and thread bodies: mg_redistribute_layout.h) ----
#include "mg_redistribute_layout.h"

// one launch of form MGR_ROWS / MGR_TILE / MGR_GATHER on `stream` of the current device: fills the a.nCells destination cells of
// `a` (element size es = 2 / 4 / 8 bytes; laneBytes = 16 or es, rows form only); `a` went through mgr_finish_args
hipError_t mg_redistribute(const MgrArgs& a, int form, int es, int laneBytes, hipStream_t stream);

constexpr int kMgrTableWords = 256; // 8-byte words of a cell table per launch of the table writer (2 KiB of kernel arguments)
struct MgrTableChunk {
    uint64_t word[kMgrTableWords];
    uint64_t* dst;
    int n;
};
// dst[0 .. bytes) = words[0 .. bytes rounded up to 8): the cell tables of a call with more than kMgrArgCells cells go to the device
// workspace by kernel arguments, in stream order and without any host buffer that would have to outlive the call
hipError_t mg_redistribute_table(void* dst, const void* words, size_t bytes, hipStream_t stream);
