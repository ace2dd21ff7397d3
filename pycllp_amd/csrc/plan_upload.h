// plan_upload.h -- the one upload of a plan's tables (plan_host.h PlanBlob): what wreg_plan_create*, big_plan_create and
// sparse_init_host do once their tables are built.  Host code only.
#ifndef PYCLLP_PLAN_UPLOAD_H
#define PYCLLP_PLAN_UPLOAD_H
#include <hip/hip_runtime.h>
#include "plan_host.h"

// *dev <- a device copy of the blob, complete when the call returns; on an error nothing stays allocated and *dev is null
inline hipError_t plan_upload(const PlanBlob& blob, hipStream_t st, void** dev) {
    *dev = nullptr;
    hipError_t e = hipMalloc(dev, blob.bytes.size());
    if (e == hipSuccess) e = hipMemcpyAsync(*dev, blob.bytes.data(), blob.bytes.size(), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) { if (*dev) (void)hipFree(*dev); *dev = nullptr; }
    return e;
}
#endif
