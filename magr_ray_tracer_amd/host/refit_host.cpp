// refit_host.cpp — the host restatement of rt_update_scene's refit (rth_set_primitives / rth_refit, include/rt355_host.h): the
// same rules (csrc/refit_common.h) run sequentially over the host BVH2.  Together with the existing TLAS::Build it is the ground
// truth the device update must match bit for bit, and it lets the oracle render animated frames.
#include <string>
#include <vector>
#include "../../include/rt355.h"
#include "../csrc/refit_common.h"
#include "rt_host.h"

namespace rt355 {

// Replaces primitives [first, first + count) keeping the topology (count, objType, matIdx); err receives why a call is refused.
int SetPrimitivesHost(std::vector<RtPrimitive>& prims, int32_t first, int32_t count, const RtPrimitive* in, std::string& err)
{
    if (count < 0 || (count > 0 && !in)) { err = "rth_set_primitives: bad count / NULL records"; return RT_E_INVALID; }
    if (count > 0 && (first < 0 || (int64_t)first + count > (int64_t)prims.size())) {
        err = "rth_set_primitives: range [" + std::to_string(first) + ", " + std::to_string((int64_t)first + count) + ") outside the " +
              std::to_string(prims.size()) + " primitives";
        return RT_E_INVALID;
    }
    for (int32_t i = 0; i < count; i++) {
        const RtPrimitive& o = prims[(size_t)first + (size_t)i];
        if (in[i].objType != o.objType || in[i].matIdx != o.matIdx) {
            err = "rth_set_primitives: primitive " + std::to_string(first + i) + " changes its objType / matIdx (topology must not change)";
            return RT_E_INVALID;
        }
    }
    for (int32_t i = 0; i < count; i++) prims[(size_t)first + (size_t)i] = in[i];
    return RT_OK;
}

// Refits every BLAS of `nodes` in place: children before parents (the breadth-first order walked backwards).
int RefitHost(std::vector<RtBVHNode2>& nodes, const std::vector<uint32_t>& primIdx, const std::vector<RtPrimitive>& prims,
              const std::vector<RtBVHInstance>& inst, std::string& err)
{
    if (nodes.empty() || inst.empty()) { err = "rth_refit: the scene has no BLAS (BuildBLAS comes first)"; return RT_E_INVALID; }
    refit::Topology t;
    if (const char* why = refit::build_topology(nodes.data(), (int32_t)nodes.size(), inst.data(), (int32_t)inst.size(), t)) {
        err = std::string("rth_refit: ") + why;
        return RT_E_UNSUPPORTED;
    }
    for (uint32_t i : t.leaves) {
        const RtBVHNode2& n = nodes[i];
        if ((uint64_t)n.first + n.count > primIdx.size()) { err = "rth_refit: a leaf range exceeds primIdx"; return RT_E_INVALID; }
        for (uint32_t s = n.first; s < n.first + n.count; s++)
            if (primIdx[s] >= prims.size()) { err = "rth_refit: primIdx out of range"; return RT_E_INVALID; }
    }
    for (size_t k = t.order.size(); k-- > 0;) {
        RtBVHNode2& n = nodes[t.order[k]];
        if (n.count > 0) refit::set_box(n, refit::leaf_box(prims.data(), primIdx.data(), n.first, n.count));
        else refit::set_box(n, lbvh::box_union(refit::node_box(nodes[n.first]), refit::node_box(nodes[n.first + 1])));
    }
    return RT_OK;
}

} // namespace rt355
