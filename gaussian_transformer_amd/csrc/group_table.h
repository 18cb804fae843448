// group_table.h -- what the apply passes of density.hip and mcmc.hip share, one copy of each: both write the parameter and the two
// Adam moments of every group in ONE launch over (row, column), from a table of groups that the caller hands in.
//   device: the group record of both kernel-argument structs (they keep their layout), the floats of one group per block, and the
//           float64 rotation of a raw quaternion: density.hip's child_xyz forms the one row it needs, mcmc.hip's noise kernel all three.
//   host:   the filler of the table and the group refusals common to gsr_densify_apply and gsr_mcmc_apply, as templates over the public
//           group type (gsr_density_group_t and gsr_mcmc_group_t have the same fields and stay two types).  The refusals take the
//           function's name and the words that differ, and come in two calls: each function has checks of its own between them.
// Every kernel of the two files compiles to the instructions it compiled to with these lines written out in it (scripts/isa_diff.py,
// profiles/isa/group_table_refactor.txt).
// NOT shared, on purpose: the two apply kernels -- one reads a map of (row, kind) and ranks, the other from[] and hist[] under a mode,
// in place or not; one template over callables would be new kernels that nobody has measured (see map_walk.h) -- and the NULL-pointer,
// role and role-width refusals, whose conditions and texts differ in more than a word.
#pragma once
#include "gsr_host.h"
#include "gsr_internal.h"

namespace gsr {

// ---- device ----
struct GroupDev {
    const float *src, *sm, *sv;
    float *dst, *dm, *dv;
    uint32_t w;
    int role;
    unsigned first_block;        // the group's blocks are [first_block, next group's first_block): group_of_block() of gsr_internal.h
    int vec4;
};

#define GROUP_PER_BLOCK 1024       // floats of one group per block: 4 rounds of 256 lanes, or 256 lanes x 16 bytes

struct Quat64 { double r, x, y, z; };
struct Row64 { double c0, c1, c2; };
__device__ __forceinline__ Quat64 unit_quat64(double qr, double qx, double qy, double qz) {      // q / |q| of a raw [r, x, y, z]
    const double norm = sqrt(qr * qr + qx * qx + qy * qy + qz * qz);
    return Quat64{qr / norm, qx / norm, qy / norm, qz / norm};
}
// Row c of the rotation matrix; a constant c leaves one branch.  The branch stays in here: as three functions that the caller selects
// from, densify_apply_kernel came out with two more v_mul_f64.
__device__ __forceinline__ Row64 rot_row(const Quat64 &q, uint32_t c) {
    const double r = q.r, x = q.x, y = q.y, z = q.z;
    double m0, m1, m2;
    if (c == 0) { m0 = 1.0 - 2.0 * (y * y + z * z); m1 = 2.0 * (x * y - r * z); m2 = 2.0 * (x * z + r * y); }
    else if (c == 1) { m0 = 2.0 * (x * y + r * z); m1 = 1.0 - 2.0 * (x * x + z * z); m2 = 2.0 * (y * z - r * x); }
    else { m0 = 2.0 * (x * z - r * y); m1 = 2.0 * (y * z + r * x); m2 = 1.0 - 2.0 * (x * x + y * y); }
    return Row64{m0, m1, m2};
}

// ---- host ----
// Files the groups of positive width into grp[] (n_filled of them) for `rows` rows each; copy_role: the role of a plain copy, the only
// one that may take 16-byte accesses.  Returns the blocks of the launch.  Sizes, pointers and roles validated by the caller.
template <class Group>
static inline unsigned fill_group_table(int n_groups, const Group *groups, uint32_t rows, int copy_role, GroupDev *grp, int &n_filled) {
    unsigned blocks = 0;
    for (int k = 0; k < n_groups; k++) {
        const Group &h = groups[k];
        if (h.width_floats <= 0) continue;
        GroupDev &d = grp[n_filled++];
        d.src = h.src; d.sm = h.src_exp_avg; d.sv = h.src_exp_avg_sq; d.dst = h.dst; d.dm = h.dst_exp_avg; d.dv = h.dst_exp_avg_sq;
        d.w = (uint32_t)h.width_floats; d.role = h.role; d.first_block = blocks;
        const uintptr_t bits = (uintptr_t)h.src | (uintptr_t)h.dst | (uintptr_t)h.src_exp_avg | (uintptr_t)h.src_exp_avg_sq |
                               (uintptr_t)h.dst_exp_avg | (uintptr_t)h.dst_exp_avg_sq;
        d.vec4 = (h.role == copy_role && h.width_floats % 4 == 0 && (bits & 15) == 0) ? 1 : 0;
        blocks += (unsigned)(((uint64_t)rows * d.w + GROUP_PER_BLOCK - 1) / GROUP_PER_BLOCK);
    }
    return blocks;
}

// First shared refusals of group k: a negative width, and rows * width beyond 32 bits (rows_text: how the function names its row
// count).  A group of width 0 passes both; the caller skips it afterwards, as it did between the two.
template <class Group>
static inline int refuse_group_size(const char *who, int k, const Group &g, unsigned long long rows, const char *rows_text) {
    if (g.width_floats < 0) return fail(GSR_ERR_INVALID_ARGUMENT, "%s: group %d: width %d", who, k, g.width_floats);
    if (rows * (unsigned long long)g.width_floats > 0xffffffffULL)
        return fail(GSR_ERR_INVALID_ARGUMENT, "%s: group %d: %s * width must stay below 2^32", who, k, rows_text);
    return GSR_OK;
}

// Second: of the four moment pointers none or all are given; *n_given: how many were
template <class Group>
static inline int refuse_group_moments(const char *who, int k, const Group &g, int *n_given = nullptr) {
    const int nm = (g.src_exp_avg != nullptr) + (g.src_exp_avg_sq != nullptr) + (g.dst_exp_avg != nullptr) + (g.dst_exp_avg_sq != nullptr);
    if (nm != 0 && nm != 4) return fail(GSR_ERR_INVALID_ARGUMENT, "%s: group %d: the four moment pointers must all be given or all be NULL", who, k);
    if (n_given) *n_given = nm;
    return GSR_OK;
}

}  // namespace gsr
