"""A layered mesh whose cells have up to 15 faces, built in numpy from a seed.

The plan is a grid of square coarse columns.  Some of them (`centres`) stay coarse while every column
around them, diagonals included, is refined 3 x 3: a centre then borders three fine columns along
each side through hanging nodes -- a 12-node polygon with 12 lateral faces, 14 with its top and
bottom, rows of up to 15 blocks.  Coarse columns further out that touch a refined one get hanging
nodes too (6-, 8- or 10-node polygons).  A coarse column and two fine ones along one of its sides are
pairwise adjacent: the cell graph has triangles, as a Voronoi or locally refined model's has."""
import numpy as np


def refined_plan(nx=6, ny=3, centres=((1, 1), (4, 1)), h=100.0):
    """returns (xy (V, 2) lattice points, columns [ring of lattice indices, counter-clockwise], coarse
    column indices).  Lattice: (3 nx + 1) x (3 ny + 1) points of spacing h / 3."""
    centres = set(map(tuple, centres))
    refined = set()
    for (ci, cj) in centres:
        for di in (-1, 0, 1):
            for dj in (-1, 0, 1):
                q = (ci + di, cj + dj)
                if q != (ci, cj) and 0 <= q[0] < nx and 0 <= q[1] < ny and q not in centres:
                    refined.add(q)
    L = 3 * nx + 1
    jj, ii = np.meshgrid(np.arange(3 * ny + 1), np.arange(L), indexing="ij")
    xy = np.stack([ii.ravel(), jj.ravel()], axis=1) * (h / 3.0)

    def node(a, b):
        return b * L + a

    columns, coarse = [], []
    for J in range(ny):
        for I in range(nx):
            if (I, J) in refined:
                for b in range(3 * J, 3 * J + 3):
                    for a in range(3 * I, 3 * I + 3):
                        columns.append([node(a, b), node(a + 1, b), node(a + 1, b + 1), node(a, b + 1)])
                continue
            a0, b0 = 3 * I, 3 * J
            ring = []
            # bottom (left to right), right (up), top (right to left), left (down): the side's two inner lattice points
            # where the column across that side is refined
            sides = [((I, J - 1), [(a0 + t, b0) for t in range(3)]),
                     ((I + 1, J), [(a0 + 3, b0 + t) for t in range(3)]),
                     ((I, J + 1), [(a0 + 3 - t, b0 + 3) for t in range(3)]),
                     ((I - 1, J), [(a0, b0 + 3 - t) for t in range(3)])]
            for nbr, pts in sides:
                ring.append(node(*pts[0]))
                if nbr in refined:
                    ring += [node(*pts[1]), node(*pts[2])]
            if (I, J) in centres:
                coarse.append(len(columns))
            columns.append(ring)
    return xy, columns, coarse


def layered_cells(xy, columns, tops):
    """nodes (V (nl + 1), 3) and cells (layers from the top, columns in order inside a layer) of the plan extruded
    between the elevations `tops` (descending, nl + 1 of them): lower ring, then upper ring"""
    nv = xy.shape[0]
    tops = np.asarray(tops, dtype=np.float64)
    nodes = np.concatenate([np.column_stack([xy, np.full(nv, z)]) for z in tops])
    cells = []
    for lay in range(len(tops) - 1):
        for ring in columns:
            cells.append([(lay + 1) * nv + v for v in ring] + [lay * nv + v for v in ring])
    return nodes, cells


PRIMARY = {"w": [1.0e5], "we": [1.0e5, 20.0], "wce": [1.0e5, 20.0, 0.02e5], "wsce": [1.0e5, 20.0, 0.05, 0.02e5]}


def wide_case(eos="we", nx=6, ny=3, centres=((1, 1), (4, 1)), layers=3, dz=100.0, h=100.0, chunk=128, seed=7,
              top_bc=True):
    """(LocalMesh, unscaled primaries (n, np), regions, coarse cells): the refined plan in `layers` layers, a top
    Dirichlet boundary on every top-layer cell (top_bc), a few sources (seeded), hydrostatic liquid initial state"""
    from waiwera_amd import unstructured
    from waiwera_amd.mesh import liquid_density_estimate
    xy, columns, coarse = refined_plan(nx, ny, centres, h)
    tops = -dz * np.arange(layers + 1)
    nodes, cells = layered_cells(xy, columns, tops)
    nc = len(columns)
    n = len(cells)
    rng = np.random.default_rng(seed)
    top = np.asarray(PRIMARY[eos], dtype=np.float64)
    srcs = []
    for c in rng.choice(np.arange(nc, n), size=4, replace=False):
        s = dict(cell=int(c), rate=-float(rng.uniform(0.5, 2.0)), enthalpy=0.0, component=0)
        srcs.append(s)
    inj = int(rng.integers(nc, n))
    while inj in [s["cell"] for s in srcs]:
        inj = int(rng.integers(nc, n))
    srcs.append(dict(cell=inj, rate=1.0, enthalpy=1.0e5 if eos != "w" else 0.0, component=1))
    rock = np.tile(np.array([1.0e-13, 1.0e-13, 1.0e-14, 0.1, 2600.0, 2.5, 1000.0, 0.0]), (n, 1))
    rock[:, 3] = 0.08 + 0.04 * rng.random(n)
    lm = unstructured.build_mesh(nodes, cells, 3, gravity=[0.0, 0.0, -9.8], rock=rock, chunk=chunk,
                                 boundaries=[(list(range(nc)), [0.0, 0.0, 1.0], top, 1)] if top_bc else [], sources=srcs)
    depth = -lm.cell_geom[:n, 2]
    T = 20.0 + 0.05 * depth
    P = 1.0e5 + 9.8 * liquid_density_estimate(T) * depth
    prim = np.zeros((n, len(top)))
    prim[:, 0] = P
    if len(top) > 1:
        prim[:, 1] = T
    if eos == "wce":
        prim[:, 2] = 0.02 * P
    if eos == "wsce":
        prim[:, 2] = 0.05
        prim[:, 3] = 0.02 * P
    region = np.ones(n, dtype=np.int32)
    coarse_cells = [lay * nc + c for lay in range(layers) for c in coarse]
    return lm, prim, region, coarse_cells


def write_mulgraph(path, xy, columns, tops):
    """a MULgraph geometry file of the plan (vertex / column names: three base-36 characters)"""
    digits = "0123456789abcdefghijklmnopqrstuvwxyz"

    def name(k):
        return digits[(k // 1296) % 36] + digits[(k // 36) % 36] + digits[k % 36]

    used = sorted({v for ring in columns for v in ring})
    lines = ["GENER  2                                                       5.0"]
    lines.append("VERTICES")
    for v in used:
        lines.append("%3s%10.3f%10.3f" % (name(v), xy[v, 0], xy[v, 1]))
    lines.append("")
    lines.append("GRID")
    for q, ring in enumerate(columns):
        lines.append("%3s %2d" % (name(q), len(ring)))
        lines += ["%3s" % name(v) for v in ring]
    lines.append("")
    lines.append("CONNECTIONS")
    lines.append("")
    lines.append("LAYERS")
    lines.append("%3s%10.3f%10.3f" % ("atm", tops[0], tops[0]))
    for k in range(1, len(tops)):
        lines.append("%3s%10.3f%10.3f" % (name(k), tops[k], 0.5 * (tops[k - 1] + tops[k])))
    lines.append("")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
