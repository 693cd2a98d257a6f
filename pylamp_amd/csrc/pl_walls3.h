// The six walls of the 3-D box and the planes over them, host side: one name table, one axis rule and one holder for "six optional
// planes in one device buffer" (the layout is in DESIGN.md section 6c, "Wall planes").  Used by pl_3d.hip and pl_mic3.hip; no kernel
// sees any of this -- Pl3WallFlow and Heat3Planes are filled from a Walls3Planes.
#pragma once
#include <cstddef>

static const char* const walls3_names[6] = {"z0", "x0", "y0", "zL", "xL", "yL"};
// the two axes p < q other than a, in z, x, y order: the axes of a plane of the walls of axis a = w % 3
inline void walls3_axes(int a, int& p, int& q) { p = a == 0 ? 1 : 0; q = a == 2 ? 1 : 2; }
// entries of wall w's plane on the grid of gn[3] nodes: (n_p, n_q) over the wall's nodes, (n_p - 1, n_q - 1) over its faces
inline size_t walls3_count(const int gn[3], int w, bool nodes) {
    int p, q;
    walls3_axes(w % 3, p, q);
    return (size_t)(gn[p] - (nodes ? 0 : 1)) * (size_t)(gn[q] - (nodes ? 0 : 1));
}
// Six optional planes, packed in wall order into one device buffer that holds room for all six: plane w starts at off[w] and has
// off[w + 1] - off[w] entries; bit w of mask: wall w has one.  dev is allocated by the first set and freed when the planes are cleared.
struct Walls3Planes {
    double* dev = nullptr; int mask = 0; size_t off[7] = {0, 0, 0, 0, 0, 0, 0};
    const double* plane(int w) const { return (mask >> w) & 1 ? dev + off[w] : nullptr; }
    size_t count(int w) const { return off[w + 1] - off[w]; }
};
