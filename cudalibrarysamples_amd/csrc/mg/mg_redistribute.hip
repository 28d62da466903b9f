// Device code of cutensorMgCopy (gfx950): the batched block-cyclic redistribution with mode permutation.
//
// One launch runs on a destination device and fills all of that device's destination cells: blockIdx.y picks the cell (slot),
// blockIdx.x walks its rows / tiles / elements grid-stride.  Reads go to whatever device owns the source cell (peer mappings of
// cutensorMgCreate), writes are local.  The thread bodies live in mg_redistribute_layout.h, where the host replay runs them too;
// the 2-, 4- and 8-byte element sizes are all the typing there is.  Static LDS of the tile kernels: 19224 bytes (2- and 4-byte
// elements), 35864 bytes (8-byte elements) — kMgrTileLds4 / kMgrTileLds8.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "mg_kernels.h"

namespace {

template <int ES, int V>
__global__ __launch_bounds__(kMgrThreads) void mg_redistribute_rows_kernel(MgrArgs a) {
    mgr_rows_thread<ES, V>(a, blockIdx.x, blockIdx.y, threadIdx.x);
}

template <int ES>
__global__ __launch_bounds__(kMgrThreads) void mg_redistribute_gather_kernel(MgrArgs a) {
    mgr_gather_thread<ES>(a, blockIdx.x, blockIdx.y, threadIdx.x);
}

template <int ES>
__global__ __launch_bounds__(kMgrThreads) void mg_redistribute_tile_kernel(MgrArgs a) {
    __shared__ typename MgrWord<ES>::L tile[kMgrTile * kMgrPitch];
    __shared__ MgrTileEdges edges;
    for (uint64_t t = blockIdx.x; t < a.work; t += gridDim.x) {      // uniform per workgroup: the barriers are reached by all
        mgr_tile_edges(a, blockIdx.y, t, threadIdx.x, edges);
        __syncthreads();
        mgr_tile_load<ES>(a, threadIdx.x, edges, tile);
        __syncthreads();
        mgr_tile_store<ES>(a, blockIdx.y, threadIdx.x, edges, tile);
        __syncthreads();                                               // the next tile overwrites edges and tile
    }
}

__global__ __launch_bounds__(kMgrThreads) void mg_redistribute_table_kernel(MgrTableChunk c) {
    const int i = (int)threadIdx.x;
    if (i < c.n) c.dst[i] = c.word[i];
}

}  // namespace

hipError_t mg_redistribute(const MgrArgs& a, int form, int es, int laneBytes, hipStream_t stream) {
    if (a.nCells <= 0 || a.work == 0) return hipSuccess;
    const dim3 grid(a.gridX, (unsigned)a.nCells), block(kMgrThreads);
#define MGR_BY_SIZE(KERNEL)                                                                       \
    switch (es) {                                                                                 \
        case 2: KERNEL<2><<<grid, block, 0, stream>>>(a); break;                                  \
        case 4: KERNEL<4><<<grid, block, 0, stream>>>(a); break;                                  \
        case 8: KERNEL<8><<<grid, block, 0, stream>>>(a); break;                                  \
        default: return hipErrorInvalidValue;                                                     \
    }
    if (form == MGR_ROWS) {
        const bool wide = laneBytes == 16;
        switch (es) {
            case 2: if (wide) mg_redistribute_rows_kernel<2, 8><<<grid, block, 0, stream>>>(a); else mg_redistribute_rows_kernel<2, 1><<<grid, block, 0, stream>>>(a); break;
            case 4: if (wide) mg_redistribute_rows_kernel<4, 4><<<grid, block, 0, stream>>>(a); else mg_redistribute_rows_kernel<4, 1><<<grid, block, 0, stream>>>(a); break;
            case 8: if (wide) mg_redistribute_rows_kernel<8, 2><<<grid, block, 0, stream>>>(a); else mg_redistribute_rows_kernel<8, 1><<<grid, block, 0, stream>>>(a); break;
            default: return hipErrorInvalidValue;
        }
    } else if (form == MGR_TILE) {
        MGR_BY_SIZE(mg_redistribute_tile_kernel)
    } else if (form == MGR_GATHER) {
        MGR_BY_SIZE(mg_redistribute_gather_kernel)
    } else {
        return hipErrorInvalidValue;
    }
#undef MGR_BY_SIZE
    return hipGetLastError();
}

hipError_t mg_redistribute_table(void* dst, const void* words, size_t bytes, hipStream_t stream) {
    const uint64_t* w = static_cast<const uint64_t*>(words);
    uint64_t* d = static_cast<uint64_t*>(dst);
    for (size_t done = 0, n = (bytes + 7) / 8; done < n;) {
        MgrTableChunk c;
        c.n = (int)(n - done < (size_t)kMgrTableWords ? n - done : (size_t)kMgrTableWords);
        for (int i = 0; i < c.n; ++i) c.word[i] = w[done + (size_t)i];
        c.dst = d + done;
        mg_redistribute_table_kernel<<<dim3(1), dim3(kMgrThreads), 0, stream>>>(c);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        done += (size_t)c.n;
    }
    return hipSuccess;
}
