// body_motion.cpp -- the motion stage of include/dsrt.h (TEMPORAL ACCUMULATION WITH BODIES) on the host: what is refused of a DsrtBodyMotion, the table the device
// kernel takes (csrc/temporal_kernel.hip), and the CPU statement of the rule, dsrt_body_motion_host.
//
// No reference counterpart (the reference renders one rigid mesh and reconstructs nothing).  Every float operation below is a single correctly rounded one in the
// order the header writes it (the file is compiled with -ffp-contract=off); the kernel does the same arithmetic on the device and tests/_motion_model.py in numpy.
#include <cmath>
#include <cstring>

#include "host_internal.hpp"

using namespace dsrt;

int dsrt::check_body_motion(const char* fn, const DsrtBodyMotion* m) {
    const std::string where(fn);
    auto fail = [&](const char* why) { set_error(where + ": " + why); return DSRT_ERR_INVALID; };
    if (!m) return fail("null argument (DsrtBodyMotion)");
    if (!m->first_tri || !m->num_tris || !m->poses_prev || !m->poses_cur || !m->prim_id) return fail("a member of DsrtBodyMotion is NULL");
    if (m->bodies < 1 || m->bodies > DSRT_MAX_BODIES) return fail("DsrtBodyMotion.bodies must be between 1 and DSRT_MAX_BODIES");
    for (int b = 0; b < m->bodies; ++b)
        if (m->first_tri[b] < 0 || m->num_tris[b] < 0) return fail("a negative first_tri or num_tris");
    for (int a = 1; a < m->bodies; ++a)
        for (int b = a + 1; b < m->bodies; ++b) {
            const int64_t a0 = m->first_tri[a], a1 = a0 + m->num_tris[a], b0 = m->first_tri[b], b1 = b0 + m->num_tris[b];
            if (a0 < b1 && b0 < a1 && a0 < a1 && b0 < b1) return fail("the triangle ranges of two bodies overlap");
        }
    for (int i = 12; i < 12 * m->bodies; ++i)
        if (!std::isfinite(m->poses_prev[i]) || !std::isfinite(m->poses_cur[i])) return fail("a pose entry is not finite");
    return DSRT_OK;
}

void dsrt::pack_body_motion(const DsrtBodyMotion& m, BodyMotionTable& t) {
    std::memset(&t, 0, sizeof t);
    for (int b = 1; b < m.bodies; ++b) {
        t.first[b] = m.first_tri[b];
        t.count[b] = m.num_tris[b];
        const float* c = m.poses_cur + 12 * (size_t)b;
        const float* q = m.poses_prev + 12 * (size_t)b;
        bool moved = false;
        for (int i = 0; i < 12; ++i) moved |= c[i] != q[i];
        if (moved) t.moved |= 1u << b;
        std::memcpy(t.poses + 24 * (size_t)b, c, 12 * sizeof(float));
        std::memcpy(t.poses + 24 * (size_t)b + 12, q, 12 * sizeof(float));
    }
}

namespace {

// r = transpose(rotation of c) * a
inline void transpose_rows(const float* c, const float a[3], float r[3]) {
    for (int k = 0; k < 3; ++k) r[k] = (c[k] * a[0] + c[4 + k] * a[1]) + c[8 + k] * a[2];
}

bool overlap(const void* a, size_t an, const void* b, size_t bn) {
    if (!a || !b || !an || !bn) return false;
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + bn && b0 < a0 + an;
}

}  // namespace

extern "C" int dsrt_body_motion_host(const DsrtBodyMotion* motion, int n, const float* normal, const float* position, float* prev_normal, float* prev_position) {
    return guarded("dsrt_body_motion_host", [&]() -> int {
    const char* fn = "dsrt_body_motion_host";
    auto fail = [&](const char* why) { set_error(std::string(fn) + ": " + why); return DSRT_ERR_INVALID; };
    if (int rc = check_body_motion(fn, motion)) return rc;
    if (n < 0) return fail("n < 0");
    if (!normal || !position) return fail("null argument");
    for (const void* p : {(const void*)motion->prim_id, (const void*)normal, (const void*)position, (const void*)prev_normal, (const void*)prev_position})
        if ((uintptr_t)p & 3u) return fail("pointer not 4-byte aligned");
    const size_t v3 = (size_t)n * 3 * sizeof(float), v1 = (size_t)n * sizeof(int32_t);
    for (const float* out : {prev_normal, prev_position})
        if (overlap(out, v3, normal, v3) || overlap(out, v3, position, v3) || overlap(out, v3, motion->prim_id, v1)) return fail("an output range overlaps an input range");
    if (overlap(prev_normal, v3, prev_position, v3)) return fail("two output ranges overlap");
    BodyMotionTable t;
    pack_body_motion(*motion, t);
    for (int i = 0; i < n; ++i) {
        const int32_t prim = motion->prim_id[i];
        int body = 0;
        for (int b = 1; b < motion->bodies; ++b)
            if ((int64_t)prim >= t.first[b] && (int64_t)prim < (int64_t)t.first[b] + t.count[b]) body = b;
        const float* N = normal + 3 * (size_t)i;
        const float* X = position + 3 * (size_t)i;
        float n2[3] = {N[0], N[1], N[2]}, x2[3] = {X[0], X[1], X[2]};
        if (body && (t.moved >> body & 1u)) {
            const float* c = t.poses + 24 * (size_t)body;
            const float* q = c + 12;
            const float d[3] = {X[0] - c[3], X[1] - c[7], X[2] - c[11]};
            float r[3], m[3];
            transpose_rows(c, d, r);
            transpose_rows(c, N, m);
            for (int k = 0; k < 3; ++k) {
                x2[k] = ((q[4 * k] * r[0] + q[4 * k + 1] * r[1]) + q[4 * k + 2] * r[2]) + q[4 * k + 3];
                n2[k] = (q[4 * k] * m[0] + q[4 * k + 1] * m[1]) + q[4 * k + 2] * m[2];
            }
        }
        if (prev_normal) std::memcpy(prev_normal + 3 * (size_t)i, n2, sizeof n2);
        if (prev_position) std::memcpy(prev_position + 3 * (size_t)i, x2, sizeof x2);
    }
    return DSRT_OK;
    });
}
