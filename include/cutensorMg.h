/*
 * cutensorMg.h — single-process multi-GPU tensor contraction (cuTENSORMg C ABI), implemented for a
 * node of AMD Instinct MI355X GPUs connected by xGMI.
 *
 * Reconstructed from the call sites of cuTENSORMg/contraction_multi_gpu.cu in
 * NVIDIA/CUDALibrarySamples (the header itself is not in the reference tree); every declaration
 * cites the line that pins it.  One host thread drives all devices; tensors are block-cyclic
 * distributed: mode i is cut into blocks of blockSize[i] elements, block b of mode i belongs to
 * device-grid coordinate b % deviceCount[i], and grid cell (c_0, c_1, ...) — linearised first mode
 * fastest — is stored in the buffer devices[cell]/pointer[cell] (contraction_multi_gpu.cu:154-217,
 * :256-284).
 */
#ifndef CUTENSORMG_H_
#define CUTENSORMG_H_

#include <stdint.h>

#include <cutensor.h>   /* the Mg sample only includes this header and calls cutensorGetErrorString (contraction_multi_gpu.cu:43) */

#ifdef __cplusplus
extern "C" {
#endif

#define CUTENSOR_MG_DEVICE_HOST (-1)

typedef struct cutensorMgHandle*                cutensorMgHandle_t;
typedef struct cutensorMgTensorDescriptor*      cutensorMgTensorDescriptor_t;
typedef struct cutensorMgContractionDescriptor* cutensorMgContractionDescriptor_t;
typedef struct cutensorMgContractionFind*       cutensorMgContractionFind_t;
typedef struct cutensorMgContractionPlan*       cutensorMgContractionPlan_t;

typedef enum {
    CUTENSORMG_ALGO_DEFAULT = -1   /* contraction_multi_gpu.cu:237 */
} cutensorMgAlgo_t;

/* contraction_multi_gpu.cu:151, :383 */
cutensorStatus_t cutensorMgCreate(cutensorMgHandle_t* handle, uint32_t numDevices, const int32_t devices[]);
cutensorStatus_t cutensorMgDestroy(cutensorMgHandle_t handle);

/* contraction_multi_gpu.cu:195-197 — elementStride / blockStride NULL = packed */
cutensorStatus_t cutensorMgCreateTensorDescriptor(const cutensorMgHandle_t handle, cutensorMgTensorDescriptor_t* desc,
                                                  uint32_t numModes, const int64_t extent[],
                                                  const int64_t elementStride[], const int64_t blockSize[],
                                                  const int64_t blockStride[], const int32_t deviceCount[],
                                                  uint32_t numDevices, const int32_t devices[], cudaDataType_t type);
cutensorStatus_t cutensorMgDestroyTensorDescriptor(cutensorMgTensorDescriptor_t desc);

/* contraction_multi_gpu.cu:228-233 */
cutensorStatus_t cutensorMgCreateContractionDescriptor(const cutensorMgHandle_t handle, cutensorMgContractionDescriptor_t* desc,
                                                       const cutensorMgTensorDescriptor_t descA, const int32_t modesA[],
                                                       const cutensorMgTensorDescriptor_t descB, const int32_t modesB[],
                                                       const cutensorMgTensorDescriptor_t descC, const int32_t modesC[],
                                                       const cutensorMgTensorDescriptor_t descD, const int32_t modesD[],
                                                       cutensorComputeType_t compute);
cutensorStatus_t cutensorMgDestroyContractionDescriptor(cutensorMgContractionDescriptor_t desc);

/* contraction_multi_gpu.cu:236-237 */
cutensorStatus_t cutensorMgCreateContractionFind(const cutensorMgHandle_t handle, cutensorMgContractionFind_t* find,
                                                 const cutensorMgAlgo_t algo);
cutensorStatus_t cutensorMgDestroyContractionFind(cutensorMgContractionFind_t find);

/* contraction_multi_gpu.cu:241-242 — one size per handle device, plus a pinned-host size */
cutensorStatus_t cutensorMgContractionGetWorkspace(const cutensorMgHandle_t handle, const cutensorMgContractionDescriptor_t desc,
                                                   const cutensorMgContractionFind_t find, cutensorWorksizePreference_t preference,
                                                   int64_t deviceWorkspaceSize[], int64_t* hostWorkspaceSize);

/* contraction_multi_gpu.cu:249-250 */
cutensorStatus_t cutensorMgCreateContractionPlan(const cutensorMgHandle_t handle, cutensorMgContractionPlan_t* plan,
                                                 const cutensorMgContractionDescriptor_t desc, const cutensorMgContractionFind_t find,
                                                 const int64_t deviceWorkspaceSize[], int64_t hostWorkspaceSize);
cutensorStatus_t cutensorMgDestroyContractionPlan(cutensorMgContractionPlan_t plan);

/* contraction_multi_gpu.cu:328-332 — pointer arrays have one entry per grid cell of the respective
 * tensor; workspaceDevice / streams have one entry per handle device.  Asynchronous: returns after
 * enqueueing on the given streams; the caller synchronises every device (:334-338). */
cutensorStatus_t cutensorMgContraction(const cutensorMgHandle_t handle, const cutensorMgContractionPlan_t plan,
                                       const void* alpha, const void* A[], const void* B[], const void* beta,
                                       const void* C[], void* D[], void* workspaceDevice[], void* workspaceHost,
                                       cudaStream_t streams[]);

/*
 * Copy between block-cyclic layouts: dst[modesDst] = src[modesSrc] for every index of the valid index space, a pure copy with a
 * permutation of modes (no scalar, no operator).  These declarations follow cuTENSORMg's public API; the reference tree never
 * calls them, so no sample line pins them.
 *
 * Both tensors are block-cyclic as cutensorMgCreateTensorDescriptor defines them, with any block sizes, device counts, ragged
 * extents and element / block strides on either side.  Elements of destination cells that belong to no valid index (padding of
 * ragged extents, gaps of non-packed strides) are not written; source padding is never read into a valid element.  Overlapping
 * source and destination cells are undefined.
 *
 * Accepted: fp16, bf16, fp32, fp64, both tensors of one type, up to 16 modes, positive strides, padded extents below 2^31.
 * INVALID_VALUE: the label sets differ, a label's extent differs, a label is repeated in one tensor.  NOT_SUPPORTED: different
 * data types, more than 16 modes, a destination cell on a device that is not in the handle (the launch that fills a cell runs on
 * that cell's device and stream; source cells may live anywhere) and, at plan creation on a handle with real devices, a (source
 * owner, destination device) pair without peer access: remote cells are read in place, and plan creation enables the peer mapping
 * of exactly the pairs the plan reads across (a source device outside the handle included).  CUTENSOR_LOG_LEVEL=1 names the reason.
 *
 * Workspace: hostWorkspaceSize is 0; deviceWorkspaceSize[g] is 0 unless the source has, or handle device g owns, more than 128
 * cells (the cell tables then go through the device workspace on that device's stream).  With all sizes 0 the call accepts null
 * workspaces.  A too-small size at plan creation is INSUFFICIENT_WORKSPACE.
 *
 * cutensorMgCopy: ptrDst / ptrSrc have one entry per grid cell of the respective tensor, deviceWorkspace / streams one per handle
 * device.  Asynchronous.  The call runs behind everything already enqueued on every stream of `streams`, and every stream of
 * `streams` ends behind the call's last access to any cell (the fork / join of cutensorMgContraction): it does not matter which of
 * the streams produced a source cell — one on a device outside the handle included — or goes on to use a cell.  deviceWorkspace[g],
 * where its size is not 0, must be 8-byte aligned.  The plan must be used with the handle it was created on (INVALID_VALUE
 * otherwise) but may outlive it until it is destroyed.
 */
typedef struct cutensorMgCopyDescriptor* cutensorMgCopyDescriptor_t;
typedef struct cutensorMgCopyPlan*       cutensorMgCopyPlan_t;

cutensorStatus_t cutensorMgCreateCopyDescriptor(const cutensorMgHandle_t handle, cutensorMgCopyDescriptor_t* desc,
                                                const cutensorMgTensorDescriptor_t descDst, const int32_t modesDst[],
                                                const cutensorMgTensorDescriptor_t descSrc, const int32_t modesSrc[]);
cutensorStatus_t cutensorMgDestroyCopyDescriptor(cutensorMgCopyDescriptor_t desc);
cutensorStatus_t cutensorMgCopyGetWorkspace(const cutensorMgHandle_t handle, const cutensorMgCopyDescriptor_t desc,
                                            int64_t deviceWorkspaceSize[], int64_t* hostWorkspaceSize);
cutensorStatus_t cutensorMgCreateCopyPlan(const cutensorMgHandle_t handle, cutensorMgCopyPlan_t* plan,
                                          const cutensorMgCopyDescriptor_t desc,
                                          const int64_t deviceWorkspaceSize[], int64_t hostWorkspaceSize);
cutensorStatus_t cutensorMgDestroyCopyPlan(cutensorMgCopyPlan_t plan);
cutensorStatus_t cutensorMgCopy(const cutensorMgHandle_t handle, const cutensorMgCopyPlan_t plan,
                                void* ptrDst[], const void* ptrSrc[],
                                void* deviceWorkspace[], void* hostWorkspace, cudaStream_t streams[]);

#ifdef __cplusplus
}
#endif

#endif /* CUTENSORMG_H_ */
