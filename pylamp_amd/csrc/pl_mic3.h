// What pl_mic3.hip (3-D marker-in-cell) and pl_3d.hip (the 3-D context) need of each other.
#pragma once
#include "pl_internal.h"
#include "pl_step3.h"

struct Pl3HostView {
    int device; hipStream_t stream; int nranks;
    int gn[3]; const double* coord[3];      // the context's node grid (host copies)
    Pl3WallFlow wallflow;                   // the flow through the walls as it is set right now (the inflow rule of the refill reads it)
    void** slot;                            // opaque state owned by pl_mic3.hip, released by pl3_mic_free
};
int  pl3_host_view(pl3_ctx* ctx, Pl3HostView* v);
int  pl3_fail(pl3_ctx* ctx, const std::string& m);
void pl3_mic_free(void** slot);
