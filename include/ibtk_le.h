/*
 * ibtk_le.h -- C-ABI of the MI355X-native Lagrangian-Eulerian coupling path.
 *
 * This library replaces the Fortran kernels behind IBTK::LEInteractor
 * (ibtk/src/lagrangian/LEInteractor.cpp, ibtk/src/lagrangian/fortran/
 * lagrangian_interaction{2,3}d.f.m4) with hand-written CDNA4 (gfx950) HIP
 * kernels.  Three levels are exported:
 *
 *  1. Device-resident API (ibtk_le_*): every array pointer is a device pointer;
 *     work is stream-ordered on the context's HIP stream; nothing blocks unless
 *     the function says so.  This is the level bench.py measures.
 *  2. Fortran-symbol host shims (lagrangian_<kernel>_{interp,spread}{2,3}d_):
 *     the exact symbols and by-reference signatures LEInteractor.cpp:68-619
 *     declares (IBTK_FC_FUNC_ lowercase + trailing underscore), host memory in
 *     and out (H2D -> kernel -> D2H).  Drop-in for the Fortran objects.
 *  3. A C++ LEInteractor facade (include/ibtk_le/LEInteractor.h) over light
 *     patch/data views, mirroring ibtk/include/ibtk/LEInteractor.h:100-993.
 *
 * Error convention (replaces TBOX_ERROR aborts, LEInteractor.cpp:679,2421,2740):
 * every function returns an ibtk_le_status; ibtk_le_last_error() describes the
 * most recent failure of the calling thread.
 */
#ifndef IBTK_LE_H
#define IBTK_LE_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes -------------------------------------------------------- */
typedef enum {
    IBTK_LE_OK = 0,
    IBTK_LE_ERR_UNKNOWN_KERNEL = 1, /* LEInteractor.cpp:679 "Unknown kernel function"        */
    IBTK_LE_ERR_GHOST_WIDTH = 2,    /* LEInteractor.cpp:2421, 2740 "insufficient ghost cells" */
    IBTK_LE_ERR_DEPTH = 3,          /* LEInteractor.cpp:769, 1627 side/edge depth mismatch   */
    IBTK_LE_ERR_ARG = 4,            /* invalid argument (null pointer, bad dim, bad box)     */
    IBTK_LE_ERR_DEVICE = 5,         /* HIP runtime error                                     */
    IBTK_LE_ERR_NOMEM = 6,          /* device allocation failed                              */
    IBTK_LE_ERR_RANGE = 7,          /* index space too large for the 32-bit bin keys         */
    IBTK_LE_ERR_INVARIANT = 8       /* a device-side consistency check failed                */
} ibtk_le_status;

/* ---- kernel functions (LEInteractor::getStencilSize, LEInteractor.cpp:668-682) */
typedef enum {
    IBTK_LE_KERNEL_PIECEWISE_CONSTANT = 0,
    IBTK_LE_KERNEL_DISCONTINUOUS_LINEAR = 1,
    IBTK_LE_KERNEL_PIECEWISE_LINEAR = 2,
    IBTK_LE_KERNEL_PIECEWISE_CUBIC = 3,
    IBTK_LE_KERNEL_IB_3 = 4,
    IBTK_LE_KERNEL_IB_4 = 5,
    IBTK_LE_KERNEL_IB_4_W8 = 6,
    IBTK_LE_KERNEL_IB_6 = 7,
    IBTK_LE_KERNEL_BSPLINE_4 = 8, /* not in the reference: cubic B-spline */
    IBTK_LE_KERNEL_USER_DEFINED = 9 /* LEInteractor::s_kernel_fcn: ibtk_le_user_interp / ibtk_le_user_spread */
} ibtk_le_kernel;

/* ---- data centerings (SAMRAI pdat::{Cell,Side,Node,Edge}Data) ---------------- */
typedef enum {
    IBTK_LE_CELL = 0, /* one array, depth q_depth, unshifted frame                      */
    IBTK_LE_SIDE = 1, /* NDIM arrays (one per axis), depth 1, x_lower[axis] -= dx/2     */
    IBTK_LE_NODE = 2, /* one array, depth q_depth, x_lower -= dx/2 in every dim         */
    IBTK_LE_EDGE = 3  /* 3D only: NDIM arrays, every dim but `axis` shifted             */
} ibtk_le_centering;

/* Patch geometry: the cell box, the ghost width of the Eulerian data and the
 * Cartesian patch geometry (CartesianPatchGeometry::getDx/getXLower/getXUpper).
 *
 * pitch: the layout of the Eulerian arrays in device memory.  {0, 0} is SAMRAI's
 * ArrayData layout, every array packed to its own ghosted extent (n0, n1, n2).
 * Otherwise every array of the patch (each side axis, each depth) has row stride
 * pitch[0] >= n0 and plane stride pitch[0] * pitch[1] (pitch[1] >= n1; 0 = n1);
 * depth k of a cell/node array starts k * pitch[0] * pitch[1] * n2 elements in.
 * With pitch[0] a multiple of 16 and 128-byte aligned array pointers, every
 * 32-point column row the 3-D sweeps stream is two whole 128-byte lines (the
 * sweeps' columns start at ilower - gcw + a multiple of 16 in x).  3-D single-
 * patch calls honour it; the level calls, the 2-D calls, ibtk_le_mark_stencils'
 * masks and the host Fortran shims take packed arrays only (pitch {0, 0}). */
typedef struct {
    int ndim;          /* 2 or 3 */
    int ilower[3];     /* patch box lower (cell indices) */
    int iupper[3];     /* patch box upper (inclusive)   */
    int gcw[3];        /* ghost cell width of the Eulerian arrays */
    double dx[3];
    double x_lower[3];
    double x_upper[3];
    int pitch[2];      /* array row / plane pitch in elements; {0, 0} = packed */
} ibtk_le_patch_geom;

typedef struct ibtk_le_ctx_s* ibtk_le_ctx;
typedef struct ibtk_le_markers_s* ibtk_le_markers;

/* ---- kernel-string helpers ---------------------------------------------------- */
/* Returns the kernel id for "IB_4", "IB_6", ... or -1 (LEInteractor.cpp:668-682). */
int ibtk_le_kernel_from_name(const char* name);

/* The USER_DEFINED kernel function: LEInteractor::s_kernel_fcn and
 * s_kernel_fcn_stencil_size (LEInteractor.h:100-101, LEInteractor.cpp:651-652), a
 * host function phi(r) of the signed distance in grid spacings, IB_4's
 * (ib4_kernel_fcn, LEInteractor.cpp:629-648) with stencil size 4 until set.
 * fcn == NULL restores the default.  Any stencil_size >= 1 (the spread's per-call
 * contribution count n * S^NDIM must stay below 2^31). */
typedef double (*ibtk_le_user_kernel_fn)(double r);
/* IB_4's kernel function, the reference's default s_kernel_fcn (ib4_kernel_fcn,
 * LEInteractor.cpp:629-651). */
double ibtk_le_ib4_kernel_fcn(double r);
int ibtk_le_set_user_kernel(ibtk_le_user_kernel_fn fcn, int stencil_size);
int ibtk_le_user_kernel(ibtk_le_user_kernel_fn* fcn, int* stencil_size);
const char* ibtk_le_kernel_name(int kernel);
/* LEInteractor::getStencilSize / getMinimumGhostWidth (LEInteractor.cpp:668-687). */
int ibtk_le_stencil_size(int kernel);
int ibtk_le_min_ghost_width(int kernel);
const char* ibtk_le_last_error(void);
const char* ibtk_le_version(void);

/* ---- context -------------------------------------------------------------------- */
/* `stream` is a hipStream_t (NULL = the default stream).  The context caches the
 * workspace the binning and sort steps need, so repeated calls allocate nothing. */
int ibtk_le_ctx_create(int device, void* stream, ibtk_le_ctx* out);
int ibtk_le_ctx_destroy(ibtk_le_ctx ctx);
int ibtk_le_ctx_set_stream(ibtk_le_ctx ctx, void* stream);
/* Restricts the next 3-D interp / spread calls on this context to a subset of
 * their work items (mode 1: the items whose planes -- interp: the planes it reads,
 * spread: the planes it owns -- all lie in [zlo, zhi], absolute z indices; mode 2:
 * the other items; mode 0: every item, the default).  A z-slab rank computes
 * its interior items while the halo exchange is in flight and the boundary
 * items after it; the two calls together equal one unrestricted call bit for
 * bit (each grid point is owned by exactly one item).  While zlo <= zhi, the
 * markers binned on this context (any mode) cut their sweep items at the
 * window's edges, so the boundary items are only the planes next to them.
 * 2-D calls ignore the window.  Replaces no reference entry point: the
 * reference overlaps nothing (RefineSchedule::fillData, LDataManager.cpp:748). */
int ibtk_le_ctx_set_plane_window(ibtk_le_ctx ctx, int mode, int zlo, int zhi);
/* Waits for the context stream and reports device-side invariant failures
 * latched by earlier calls (IBTK_LE_ERR_INVARIANT), then clears them: flag 1 / 2 a
 * stencil left its staged region / bin bounds, 4 an interior list entry missing from a
 * level's binned lists, 8 a fixed-capacity migration overflowed, 16 a 3-D spread's
 * candidate stream reached 2^31 entries (it holds up to 4 sorted positions a marker,
 * 16 bytes of device memory a marker, kept with the binning), 32 the spread fluid sources
 * do not integrate to their strengths, or the boundary offset does not cancel them
 * (ibtk_le_source_normalize), flag 64 a flow meter's web is wider than the plan's max_web_nodes
 * (ibtk_le_meters_update). */
int ibtk_le_ctx_synchronize(ibtk_le_ctx ctx);

/* ---- marker binning (device LIndexSetData / LDataManager re-binning) --------------
 * Replaces the per-patch index bookkeeping LEInteractor::buildLocalIndices
 * (LEInteractor.cpp:3031-3108) hands to the Fortran: it takes the list of
 * (local marker index, periodic shift) pairs -- `indices_dev`/`Xshift_dev`, or
 * NULL/NULL for the identity list 0..n-1 with zero shifts -- and sorts it on the
 * device by the stencil anchor cell of X(s)+Xshift (stable radix sort; 3-D:
 * buckets of (anchor plane, 32x16-cell column, reach band); 2-D: bricks of 16^2
 * cells).  The handle keeps device copies of the sorted list, and a pointer to its
 * context: destroy a context's markers before the context.
 * A binning refused before any device allocation or launch (argument, geometry and range
 * checks) leaves the handle exactly as it was; one that fails later (NOMEM, a HIP error)
 * leaves it unbinned: interp, spread and rebin return IBTK_LE_ERR_ARG until the next binning. */
int ibtk_le_markers_create(ibtk_le_ctx ctx, ibtk_le_markers* out);
int ibtk_le_markers_destroy(ibtk_le_markers m);
int ibtk_le_markers_bin(ibtk_le_ctx ctx, ibtk_le_markers m, const ibtk_le_patch_geom* geom, int kernel,
                        const double* X_dev, const int* indices_dev, const double* Xshift_dev, int nindices);
/* The same for a fixed-capacity marker array whose length lives on the device
 * (*n_dev <= capacity; a migration's output, no host sync): rows [n_dev, capacity)
 * are binned outside -- interp writes 0 to their Q rows, spread skips them -- so
 * Q/F arrays must hold capacity rows.  3-D, identity list. */
int ibtk_le_markers_bin_count(ibtk_le_ctx ctx, ibtk_le_markers m, const ibtk_le_patch_geom* geom, int kernel,
                              const double* X_dev, int capacity, const int* n_dev);
/* Re-bin the list of the last ibtk_le_markers_bin / _bin_count / ibtk_le_level_bin call
 * on `m` (same entries, shifts, patches and kernel) at new positions X_dev (the
 * markers moved, as between two steps of IBMethod's explicit loop).  The result --
 * sorted order, bucket starts, sorted positions, sweep items -- is exactly that of
 * binning again, but it is computed from the previous order: the entries whose
 * bucket did not change keep their relative order and the others are inserted
 * (with nothing moved, one pass over the list).  No host sync.  Replaces the
 * per-step re-binning of LDataManager's LIndexSetData (LDataManager.cpp:1446-1493,
 * IndexUtilities-inl.h:66-89) after a position update.  After ibtk_le_markers_bin_count
 * the re-binning reads the device count n_dev of that call again: it must stay valid
 * (and hold the list's length) until the next full binning of `m`. */
int ibtk_le_markers_rebin(ibtk_le_ctx ctx, ibtk_le_markers m, const double* X_dev);
/* Number of list entries, and device pointers to the sorted list (entry -> marker
 * index, and entry -> Xshift[NDIM]); valid until the next bin call. */
int ibtk_le_markers_count(ibtk_le_markers m);
/* Device pointer to the canonical order: order_dev[i] = position in the binned
 * list (0..count-1) of the i-th entry in canonical order.  Valid until the next
 * bin call; the caller may copy it to the host to feed the oracle the same list. */
int ibtk_le_markers_order(ibtk_le_markers m, const int** order_dev);

/* ---- interpolation / spreading on device-resident data --------------------------
 * q_dev[c] points at the ghosted Fortran-ordered array of component c:
 *   SIDE/EDGE: c = 0..NDIM-1, the array of axis c (SideData::getPointer(c)), depth 1
 *   CELL/NODE: c = 0 only, an array of depth q_depth (depth slowest)
 * Q_dev is the marker array in LData layout: AoS, Q_depth values per marker
 * (SIDE/EDGE: Q_depth == NDIM).  X_dev: AoS NDIM positions per marker.
 * The marker list is the one last binned into `m` (same kernel and geometry).
 * A list may name a marker several times (LIndexSetData's ghost-box list holds
 * its periodic images): spread adds every entry; interp writes Q(:, s) from the
 * LAST entry naming s, as the Fortran's sequential l-loop overwrites it.
 *
 * interp:  Q(d, s) = sum_i w_i(X(s)+Xshift) q(i, d)   for every listed s
 *          (LEInteractor.cpp:970-1055 / lagrangian_<k>_interp3d, f.m4:1258-1385)
 * spread:  q(i, d) += sum_s w_i(X(s)+Xshift) Q(d, s) / (dx0 dx1 [dx2])
 *          summed per grid point in a fixed order (work-item-private LDS
 *          accumulation, no global atomics): deterministic and bit-stable run
 *          to run
 *          (LEInteractor.cpp:1828-1913 / lagrangian_<k>_spread3d, f.m4:1395-1522) */
int ibtk_le_interp(ibtk_le_ctx ctx, ibtk_le_markers m, int kernel, int centering, int axis,
                   const ibtk_le_patch_geom* geom, const double* const* q_dev, int q_depth, double* Q_dev,
                   int Q_depth, const double* X_dev);
int ibtk_le_spread(ibtk_le_ctx ctx, ibtk_le_markers m, int kernel, int centering, int axis,
                   const ibtk_le_patch_geom* geom, double* const* q_dev, int q_depth, const double* Q_dev,
                   int Q_depth, const double* X_dev);

/* USER_DEFINED interpolation and spreading: LEInteractor::userDefinedInterpolate /
 * userDefinedSpread (LEInteractor.cpp:3141-3266, 3268-3393), the branches of the
 * private interpolate()/spread() at :2688 and :3007.  Arguments as ibtk_le_interp /
 * ibtk_le_spread, with the list given directly (no binning): indices_dev (n list
 * entries -> marker, NULL: entry l is marker l) and Xshift_dev (n x NDIM, NULL:
 * zero).  Per entry and dimension: stencil centre floor((X+Xshift-x_lower)/dx) +
 * ilower; an even stencil starts below or above it as the UNSHIFTED X lies below
 * or above the cell centre (:3188, as the reference compares); the stencil is
 * clipped into the ghost box; weights phi((X+Xshift - x_i)/dx).  phi is a host
 * function: the host evaluates it (one synchronization per call), the device
 * sums.  interp: Q(d, s) = sum w0 w1 [w2] q in the reference's loop order (the
 * last entry naming s writes it); spread: q += w0 w1 [w2] Q(d, s) / (dx0 dx1
 * [dx2]), every grid point summed in list order (bit-stable; the reference's
 * sequential order). */
int ibtk_le_user_interp(ibtk_le_ctx ctx, int centering, int axis, const ibtk_le_patch_geom* geom,
                        const double* const* q_dev, int q_depth, double* Q_dev, int Q_depth, const double* X_dev,
                        const int* indices_dev, const double* Xshift_dev, int n);
int ibtk_le_user_spread(ibtk_le_ctx ctx, int centering, int axis, const ibtk_le_patch_geom* geom,
                        double* const* q_dev, int q_depth, const double* Q_dev, int Q_depth, const double* X_dev,
                        const int* indices_dev, const double* Xshift_dev, int n);

/* Density-weighted spread, f += S (F ds): LDataManager::spread with ds_data
 * (LDataManager.cpp:398-470), which forms F_ds[k][d] = F[k][d] * ds[k] and then
 * spreads it.  ds_dev holds one double per marker (indexed like Q_dev's markers).
 * The product is formed in the gather that stages F for the spread kernel, so it
 * costs no extra pass; the values spread are the rounded products, as in the
 * reference. */
int ibtk_le_spread_ds(ibtk_le_ctx ctx, ibtk_le_markers m, int kernel, int centering, int axis,
                      const ibtk_le_patch_geom* geom, double* const* q_dev, int q_depth, const double* Q_dev,
                      int Q_depth, const double* ds_dev, const double* X_dev);

/* ---- a level of patches (3-D) ------------------------------------------------------
 * LDataManager::spread / interp loop over the patches of a level, one LEInteractor
 * call per patch (LDataManager.cpp:625-660, 763-807).  Here one launch per sweep
 * covers every patch: the patches' lists are binned together (bucket ranges per
 * patch, one device sort) and the sweep items of all patches form one table.
 * geoms[q]: patch q's box, ghost width and geometry (one dx for the level);
 * entry_offsets (host, npatch + 1): patch q's list is entries [off[q], off[q+1])
 * of indices_dev / Xshift_dev (NULL/NULL: entry l is marker l, no shift) -- the
 * interior list for interp, the ghost-box list for spread, as LDataManager uses.
 * q_dev: the arrays of patch 0, then patch 1, ... (NDIM per patch for SIDE/EDGE,
 * one for CELL/NODE).  Results equal the per-patch calls' (interp bit for bit;
 * spread in each patch's own fixed order).
 * Limit: a level interp / spread / zero_spread / fill_interp takes at most 4
 * components (CELL / NODE: q_depth <= 4); more returns IBTK_LE_ERR_ARG ("level calls
 * take at most 4 components") and writes nothing.
 * ibtk_le_level_bin fails as ibtk_le_markers_bin does: refused before any device allocation
 * or launch (argument, geometry and range checks of every patch), the handle is exactly as it
 * was; failing later (NOMEM, a HIP error), it is unbinned and later calls return IBTK_LE_ERR_ARG. */
int ibtk_le_level_bin(ibtk_le_ctx ctx, ibtk_le_markers m, int npatch, const ibtk_le_patch_geom* geoms, int kernel,
                      const double* X_dev, const int* entry_offsets, const int* indices_dev,
                      const double* Xshift_dev);
int ibtk_le_level_interp(ibtk_le_ctx ctx, ibtk_le_markers m, int kernel, int centering, int axis,
                         const double* const* q_dev, int q_depth, double* Q_dev, int Q_depth, const double* X_dev);
int ibtk_le_level_spread(ibtk_le_ctx ctx, ibtk_le_markers m, int kernel, int centering, int axis,
                         double* const* q_dev, int q_depth, const double* Q_dev, int Q_depth, const double* X_dev);
/* q := 0 on every patch array (ghosts included), then ibtk_le_level_spread, in one
 * launch: LDataManager::spread's setToScalar(f, 0, interior_only = false) fused with
 * its patch loop (LDataManager.cpp:588-654).  The sweep's items start their owned
 * points from 0 instead of reading them; items no marker reaches store zeros.
 * Bitwise ibtk_le_level_zero followed by ibtk_le_level_spread. */
int ibtk_le_level_zero_spread(ibtk_le_ctx ctx, ibtk_le_markers m, int kernel, int centering, int axis,
                              double* const* q_dev, int q_depth, const double* Q_dev, int Q_depth,
                              const double* X_dev);
/* One binning for both sweeps: m binned on the ghost-box lists (the spread's), then
 * told the interior lists (interior_offsets on the host, npatch + 1; indices on the
 * device; markers 0 .. n_markers-1): later level interps on m write Q only from the
 * entries the interior lists name (each patch's interior list is the unshifted
 * sub-list of its ghost-box list whose cells lie in the patch box, LIndexSetData.cpp:
 * 111-166), so results equal interp over a binning of the interior lists bit for bit.
 * Cleared by the next bin.  An interior entry missing from its patch's binned list
 * raises device flag 4 (ibtk_le_ctx_synchronize).  After ibtk_le_markers_rebin, a call
 * with the same offsets, index pointer and n_markers as the last one since the last
 * full binning is a no-op on the device when no marker changed bucket (the lists are
 * taken to be unchanged between binnings, as the re-binning takes the binned ones). */
int ibtk_le_level_select_interior(ibtk_le_ctx ctx, ibtk_le_markers m, int n_markers, const int* interior_offsets,
                                  const int* interior_indices_dev);
/* Forget the selection kept by ibtk_le_level_select_interior: the next call recomputes it
 * whatever its arguments (a caller that rewrites the interior lists in place, or frees them
 * and allocates new ones, calls this first). */
int ibtk_le_level_select_interior_reset(ibtk_le_markers m);
/* Zeroes every patch array of a level, ghosts included, in one launch: the
 * f := 0 before LDataManager::spread accumulates into the level (its
 * f_data_ops->setToScalar(f_data_idx, 0.0, interior_only = false),
 * LDataManager.cpp:596).  q_dev as
 * ibtk_le_level_fill_ghosts (NDIM arrays per patch for SIDE / EDGE; one array of
 * depth q_depth for CELL / NODE), each contiguous. */
int ibtk_le_level_zero(ibtk_le_ctx ctx, int npatch, const ibtk_le_patch_geom* geoms, int centering,
                       double* const* q_dev, int q_depth);
/* Ghost fill of a level of equal patches tiling a box, periodic in the dims
 * periodic[d] != 0 (NULL: all): every ghost point of every patch array takes the
 * value of the patch owning its (wrapped) index -- the RefineSchedule::fillData
 * LDataManager::interp runs before interpolating (LDataManager.cpp:748-751).
 * SIDE (NDIM arrays per patch; the face shared by two patches is the upper
 * patch's) or CELL (one array of depth q_depth per patch). */
int ibtk_le_level_fill_ghosts(ibtk_le_ctx ctx, int npatch, const ibtk_le_patch_geom* geoms, int centering,
                              double* const* q_dev, int q_depth, const int* periodic);
/* ibtk_le_level_fill_ghosts(m's patches, periodic) followed by ibtk_le_level_interp,
 * Q bit for bit, in one sweep: a patch's ghost point is read in the neighbour patch the
 * fill would copy it from (the patch owning its wrapped index, at the same global
 * index), so no ghost value is written (across a non-periodic face, where the fill
 * copies nothing, the patch's own ghost values are read).  Fused when, per component, every patch's array lies within one 2-GB
 * address window (one allocation per component for the level, e.g.), the patches have
 * at least 32 + W - 1 cells in x and 16 + W - 1 in y (W: the kernel's stencil width),
 * and the data are SIDE or CELL of depth 1; otherwise the two calls (NODE and EDGE data:
 * ibtk_le_level_fill_ghosts' IBTK_LE_ERR_ARG, "side or cell data", nothing written).
 * More than 4 components are refused before the fill writes a ghost. */
int ibtk_le_level_fill_interp(ibtk_le_ctx ctx, ibtk_le_markers m, int kernel, int centering, int axis,
                              double* const* q_dev, int q_depth, double* Q_dev, int Q_depth, const double* X_dev,
                              const int* periodic);

/* ---- helpers for a single periodic patch (uniform finest level) -----------------
 * Fill the ghost layers of the arrays of `centering` from the periodic interior
 * (the RefineSchedule::fillData the caller runs before interp, LDataManager.cpp:750). */
int ibtk_le_fill_periodic_ghosts(ibtk_le_ctx ctx, const ibtk_le_patch_geom* geom, int centering,
                                 double* const* q_dev, int q_depth, const int* periodic);
/* ibtk_le_fill_periodic_ghosts followed by ibtk_le_interp, with the same Q bit for bit,
 * in one sweep for a 3-D column binning: the interp reads every ghost point of the
 * ghost box at its periodic image in the periodic dims (the value the fill copies
 * there) and writes no ghost value (q is not modified).  periodic NULL: every dim.
 * Other binnings: the two calls. */
int ibtk_le_fill_interp(ibtk_le_ctx ctx, ibtk_le_markers m, int kernel, int centering, int axis,
                        const ibtk_le_patch_geom* geom, const double* const* q_dev, int q_depth, double* Q_dev,
                        int Q_depth, const double* X_dev, const int* periodic);
/* Spreading in ghost-region-sum mode: zero the ghost layers before spreading the
 * interior markers, then fold every ghost value back onto its periodic interior
 * image (dims folded slowest first, one source per destination per pass:
 * deterministic).  The multi-GPU path uses the same fold along x/y and an RCCL
 * exchange along z.
 * Limit: ibtk_le_fill_periodic_ghosts, ibtk_le_zero_ghosts and
 * ibtk_le_fold_periodic_ghosts take at most 16 arrays a call (CELL / NODE: q_depth
 * <= 16); more returns IBTK_LE_ERR_ARG ("too many arrays") and writes nothing. */
int ibtk_le_zero_ghosts(ibtk_le_ctx ctx, const ibtk_le_patch_geom* geom, int centering, double* const* q_dev,
                        int q_depth);
/* ibtk_le_zero_ghosts followed by ibtk_le_spread, bit for bit, in one sweep for a 3-D
 * column binning: the spread's items start their owned ghost points (outside the data
 * box) from 0 instead of reading them, and items no marker reaches store the zeros
 * (the ghost zeroing of LDataManager::spread, LDataManager.cpp:587-671, with no
 * separate pass over the ghost layers).  Other binnings: the two calls. */
int ibtk_le_zero_ghosts_spread(ibtk_le_ctx ctx, ibtk_le_markers m, int kernel, int centering, int axis,
                               const ibtk_le_patch_geom* geom, double* const* q_dev, int q_depth,
                               const double* Q_dev, int Q_depth, const double* X_dev);
/* The target as LDataManager::spread hands it to LEInteractor::spread: every point of
 * q set to 0, ghosts included (LDataManager.cpp:596, setToScalar(f, 0,
 * interior_only = false)), then ibtk_le_spread into it -- bit for bit those two steps.
 * A 3-D column binning does both in the spread's sweep (items start every owned point
 * from 0 and never read q; items no marker reaches store zeros), so q is written once
 * and not read.  Other binnings (2-D, an empty list): the zeroing (pitched arrays: the
 * whole span, row padding included), then ibtk_le_spread. */
int ibtk_le_zero_spread(ibtk_le_ctx ctx, ibtk_le_markers m, int kernel, int centering, int axis,
                        const ibtk_le_patch_geom* geom, double* const* q_dev, int q_depth, const double* Q_dev,
                        int Q_depth, const double* X_dev);
int ibtk_le_fold_periodic_ghosts(ibtk_le_ctx ctx, const ibtk_le_patch_geom* geom, int centering,
                                 double* const* q_dev, int q_depth, const int* periodic);
/* Physical-boundary ghost operators for side-centred data on one patch
 * (CartSideRobinPhysBdryOp, CartSideRobinPhysBdryOp.cpp:358-493, arithmetic of
 * cartphysbdryop{2,3}d.f.m4).  adjoint = 0: setPhysicalBoundaryConditions, the
 * ghost fill before interpolation; adjoint = 1: accumulateFromPhysicalBoundary
 * Data, the fold LDataManager::spread runs after spreading (LDataManager.cpp:
 * 655-659).  u_dev[axis]: the ghosted side arrays; the ghost width must be the
 * same in every dim (the reference asserts it, :519-527).  physical[2 d + upper]
 * flags a face on a non-periodic physical boundary (edges/corners are boxes
 * whose faces are all physical); acoef/bcoef/gcoef[c * 2 ndim + loc] are the
 * Robin coefficients of component c on face loc, constant over the face
 * (RobinBcCoefStrategy::setBcCoefs, index NDIM*depth + axis with depth 0).
 * Periodic dims are folded/filled separately (ibtk_le_{fold,fill}_periodic_
 * ghosts), before the physical fold and after the physical fill.  Bitwise equal
 * to the serial Fortran order. */
int ibtk_le_phys_bdry_side(ibtk_le_ctx ctx, const ibtk_le_patch_geom* geom, double* const* u_dev,
                           const int* physical, const double* acoef, const double* bcoef, const double* gcoef,
                           int adjoint);
/* The side-centred curl of a side-centred field on one 3-D patch, fp64:
 *   w = alpha * curl u         (accumulate == 0)
 *   w = alpha * curl u + w     (accumulate != 0)
 * over the patch's three side boxes -- PatchMathOps::curl(side, side), the arithmetic of
 * stoscurl3d (ibtk/src/math/fortran/curl3d.f.m4:457-559) -- the Eulerian operator on either
 * side of the generalized IB coupling calls: GeneralizedIBMethod::interpolateVelocity forms
 * w = 0.5 curl u before it interpolates W (GeneralizedIBMethod.cpp:292-319), spreadForce
 * adds f += 0.5 curl n after it spreads N (:537-577).  u_dev[a] / w_dev[a]: the ghosted
 * side array of axis a.  Each component is fac * (an eight-term sum taken left to right in
 * the reference's operand order), fac = 0.125 / dx[d] one division, the difference of two
 * such terms, then t = alpha * c rounded once (the reference's scale pass) and, when
 * accumulating, w = t + w rounded once (its axpy): bit for bit the reference's values, no
 * contraction.  Nothing outside the three side boxes of w is written (no ghost point, no
 * row padding) and u is never written.
 *
 * u_geom and w_geom agree in ndim (3), ilower, iupper and dx; they may differ in gcw and
 * pitch (packed and pitched layouts are honoured, as in the other 3-D single-patch calls).
 *
 * periodic: NULL or all zeros is the PLAIN ROUTINE, which is the reference's: it reads u's
 * ghost layer as it stands and needs u_geom->gcw[d] >= 1 in every dim
 * (IBTK_LE_ERR_GHOST_WIDTH otherwise).  NULL means "none" here -- unlike
 * ibtk_le_fill_periodic_ghosts and ibtk_le_fill_interp, where NULL means every dim.  Where
 * periodic[d] != 0, a read outside the cell range of dim d is taken at its periodic image
 * by ibtk_le_fill_periodic_ghosts' rule for side data (index i reads ilower + (i - ilower)
 * mod n, the face iupper + 1 of an array's own axis included): bit for bit
 * ibtk_le_fill_periodic_ghosts(u) followed by the plain call, without writing u and
 * without needing a ghost layer (or a box of 2 gcw + 1 cells) in that dim.
 *
 * IBTK_LE_ERR_ARG, with nothing written: ndim != 3; boxes or dx that differ; a null
 * pointer; any w array overlapping any u array (the curl does not run in place); a
 * non-finite or zero dx.  An empty box is IBTK_LE_OK and writes nothing.  One launch on the
 * context stream, no host synchronisation, no allocation. */
int ibtk_le_curl_side(ibtk_le_ctx ctx, const ibtk_le_patch_geom* u_geom, const double* const* u_dev,
                      const ibtk_le_patch_geom* w_geom, double* const* w_dev, double alpha, int accumulate,
                      const int* periodic);
/* Local numbering of one patch's markers (LDataManager::computeNodeDistribution,
 * LDataManager.cpp:2839-3027, cells by IndexUtilities::getCellIndex): order_dev[i]
 * is the input index of the marker given local index i.  Markers whose cell is in
 * the patch box come first, in box iteration order (x fastest), input order within
 * a cell (a stable device radix sort); the others follow in input order.  If
 * n_interior is not NULL it receives the count inside the box (this synchronises
 * the stream). */
int ibtk_le_local_numbering(ibtk_le_ctx ctx, const ibtk_le_patch_geom* geom, const double* X_dev, int n_markers,
                            int* order_dev, int* n_interior);
/* Build the list of interior markers and of their periodic images that fall in the
 * ghost box (LIndexSetData::cacheLocalIndices, LIndexSetData.cpp:83-169, for one
 * patch covering a periodic domain; getCellIndex, IndexUtilities-inl.h:66-89).
 * Order: the reference's -- the ghost box's cells in iteration order (x fastest;
 * an image sits in its shifted cell), each cell's markers by index.  Writes up to
 * `capacity` entries into indices_dev / Xshift_dev (NDIM per entry) and the
 * entry count into *count (host).  ghost = 0 gives the interior list.
 * If the list needs more than `capacity` entries, nothing is written, *count
 * holds the required size and IBTK_LE_ERR_ARG is returned.  Synchronises. */
int ibtk_le_periodic_index_list(ibtk_le_ctx ctx, const ibtk_le_patch_geom* geom, const double* X_dev,
                                int n_markers, int ghost, const int* periodic, int* indices_dev,
                                double* Xshift_dev, int capacity, int* count);
/* The same lists with the Lagrangian index of every marker (lag_dev[s]; NULL = s):
 * within a cell the entries follow the LNodeSet order, sorted by Lagrangian index
 * and uniqued (LDataManager.cpp:1487-1493: of markers sharing a cell and a Lagrangian
 * index the lowest marker index is kept; the reference leaves which one unspecified).
 * With lag_dev the entry count is known only after uniquing: a capacity below it
 * writes nothing and returns IBTK_LE_ERR_ARG with *count = the required size.
 * which = 0: every entry (d_local_petsc_indices /
 * d_periodic_shifts), 1: the cells of the patch box (d_interior_*), 2: the other
 * ghost-box cells (d_ghost_*) -- the three lists cacheLocalIndices caches.
 * SAMRAI's IndexData walks its items in insertion order; the lists take the
 * box iteration order, which that insertion order follows for sets appended
 * cell by cell (LDataManager.cpp:1446-1482 walks the cells in box order). */
int ibtk_le_index_set_list(ibtk_le_ctx ctx, const ibtk_le_patch_geom* geom, const double* X_dev, const int* lag_dev,
                           int n_markers, int ghost, const int* periodic, int which, int* indices_dev,
                           double* Xshift_dev, int capacity, int* count);
/* LEInteractor::buildLocalIndices for a box that is neither the patch box nor the
 * ghost box (LEInteractor.cpp:3070-3106): the entries of the which = 0 list above
 * whose cell -- the cell of the index set's item, an image's shifted cell -- lies in
 * [box_lo, box_hi], in the same order and with the same periodic shifts (the
 * reference's per-cell offsets, -/+ periodic_shift * dx beyond the patch's periodic
 * sides, are the images' shifts).  box == the patch box gives the which = 1 list,
 * box == the ghost box the which = 0 list.  cells_dev (NULL: not written) receives
 * NDIM ints per entry: its cell.  Count and capacity as above; synchronises. */
int ibtk_le_index_set_box_list(ibtk_le_ctx ctx, const ibtk_le_patch_geom* geom, const double* X_dev,
                               const int* lag_dev, int n_markers, int ghost, const int* periodic, const int* box_lo,
                               const int* box_hi, int* indices_dev, double* Xshift_dev, int* cells_dev, int capacity,
                               int* count);
/* The entries of a cached list whose cell (cells_dev, NDIM ints per entry, as
 * ibtk_le_index_set_box_list writes them) lies in [box_lo, box_hi], order kept:
 * buildLocalIndices' box branch over a cached index set.  Xshift_dev may be NULL
 * (then Xshift_out is not written).  Synchronises. */
int ibtk_le_list_in_box(ibtk_le_ctx ctx, int ndim, const int* cells_dev, const int* indices_dev,
                        const double* Xshift_dev, int n, const int* box_lo, const int* box_hi, int* indices_out,
                        double* Xshift_out, int capacity, int* count);
/* LDataManager::computeNodeDistribution (LDataManager.cpp:2839-3027) for one patch
 * whose marker index data has `ghost` ghost cells: order_dev[i] = the input index
 * of the marker numbered i.  The local nodes (getCellIndex cell in the patch box)
 * come first, cell by cell in box order (x fastest), each cell by Lagrangian index
 * (lag_dev; NULL = input index) with repeated (cell, Lagrangian index) pairs kept
 * once (LDataManager.cpp:1487-1493); then the nonlocal nodes of the ghost cells in
 * ghost-box order.  Markers outside the ghost box are dropped.  *n_local and
 * *n_nonlocal (host) receive the counts.  Synchronises. */
int ibtk_le_node_distribution(ibtk_le_ctx ctx, const ibtk_le_patch_geom* geom, const double* X_dev,
                              const int* lag_dev, int n_markers, int ghost, int* order_dev, int* n_local,
                              int* n_nonlocal);

/* LDataManager::computeNodeDistribution (LDataManager.cpp:2874-2947) over the local
 * patches of one level, geoms[q] in PatchLevel order: equal patch boxes aligned to one
 * tiling of the domain [dom_lo, dom_hi] (periodic in the dims periodic[d] != 0; NULL =
 * all), cells by getCellIndex in the domain frame.  X_dev holds the rank's markers (its
 * own and the ghost nodes it holds), lag_dev their Lagrangian indices (NULL = the
 * marker index).  order_dev[i] = the input index of the marker that is node i:
 *   nodes 0 .. n_local-1: the markers in a local patch's box, patch by patch, the box's
 *     cells in box order (x fastest), a cell's set by Lagrangian index and uniqued
 *     (LDataManager.cpp:1487-1493, lowest marker index kept);
 *   then n_nonlocal nodes: the markers in some patch's ghost cells (periodic images
 *     included) whose Lagrangian index no local node has, one per index, at its first
 *     sighting -- patches in order, a patch's ghost box walked in box order, skipping
 *     its patch box (SAMRAI's BoxList::removeIntersections order is not vendored: that
 *     order is the box order here, parity unpinned).
 * Markers in no patch's ghost box are not numbered.  The global PETSc index of local
 * node i is node_offset + i, node_offset = the local counts of the lower ranks
 * (computeNodeOffsets, LDataManager.cpp:3029-3047: an all-gather the caller runs).
 * Synchronises. */
int ibtk_le_level_node_distribution(ibtk_le_ctx ctx, int npatch, const ibtk_le_patch_geom* geoms, const int* dom_lo,
                                    const int* dom_hi, const int* periodic, const double* X_dev, const int* lag_dev,
                                    int n_markers, int ghost, int* order_dev, int* n_local, int* n_nonlocal);
/* LIndexSetData::cacheLocalIndices (LIndexSetData.cpp:83-169) for every local patch of a
 * level in one call: the lists LDataManager::spread / interp hand LEInteractor per patch
 * (LDataManager.cpp:634-654, 763-807).  The patches as for ibtk_le_level_node_distribution
 * (equal boxes on one tiling of [dom_lo, dom_hi], periodic[d] != 0 periodic, NULL = all);
 * cells by getCellIndex in the domain frame, without Lagrangian indices (every marker is its
 * own node).
 *   interior lists: the markers whose cell lies in patch q's box, at interior_dev
 *     [interior_off[q], interior_off[q + 1]);
 *   ghost-box lists: the markers and their periodic images whose cell lies in patch q's
 *     box grown by `ghost`, at ghost_dev / Xshift_dev (NDIM doubles an entry: the image's
 *     shift, +-(dom_hi - dom_lo + 1) dx per periodic dim) [ghost_off[q], ghost_off[q + 1]).
 * Within a patch the entries follow (order 0) its (ghost) box's cells in box order, x
 * fastest, a cell's markers by index -- ibtk_le_periodic_index_list's order for one patch,
 * the reference's IndexData order -- or (order 1) the markers' order, a marker's images in
 * image order (the same sets; a sort by patch alone, fewer radix passes).
 * interior_off / ghost_off are host arrays of npatch + 1.  If a list needs more than its
 * capacity, both offset arrays are still written (off[npatch] = the size needed), that list
 * is not, and IBTK_LE_ERR_ARG is returned.  Synchronises. */
int ibtk_le_level_index_lists(ibtk_le_ctx ctx, int npatch, const ibtk_le_patch_geom* geoms, const int* dom_lo,
                              const int* dom_hi, const int* periodic, const double* X_dev, int n_markers, int ghost,
                              int order, int* interior_dev, int interior_cap, int* interior_off, int* ghost_dev,
                              double* Xshift_dev, int ghost_cap, int* ghost_off);
/* beginDataRedistribution's wrap of marker positions into the periodic domain
 * (LDataManager.cpp:1385-1399), in place on n (ndim)-records: per periodic dim
 * (periodic NULL: all) add / subtract the domain length while outside
 * [x_lower, x_upper), then clamp every dim into [x_lower, x_upper - DBL_EPSILON]. */
int ibtk_le_wrap_positions(ibtk_le_ctx ctx, int ndim, long long n, double* X_dev, const double* x_lower,
                           const double* x_upper, const int* periodic);
/* endDataRedistribution's reorder of an LData into the new numbering (the VecScatter of
 * LDataManager.cpp:1823-1917): out[i][k] = in[order_dev[i]][k], depth doubles per
 * node, device arrays, in and out distinct. */
int ibtk_le_ldata_reorder(ibtk_le_ctx ctx, const int* order_dev, int n, const double* in_dev, int depth,
                          double* out_dev);

/* Markers whose cell (IndexUtilities::getCellIndex against the patch box) lies in
 * [box_lo, box_hi], no periodic shifts: the list LEInteractor's X-only overloads
 * build (LEInteractor.cpp:3110-3139).  Marker-major order. */
int ibtk_le_box_index_list(ibtk_le_ctx ctx, const ibtk_le_patch_geom* geom, const double* X_dev, int n_markers,
                           const int* box_lo, const int* box_hi, int* indices_dev, int capacity, int* count);

/* Marker position update, elementwise over the n = M * NDIM doubles of the
 * device arrays (any layout, as long as all four share it):
 *   IBTK_LE_EULER, IBTK_LE_MIDPOINT:  X_new = dt * U0 + X_cur
 *     (IBMethod::eulerStep / midpointStep, IBMethod.cpp:619-655: VecWAXPY with U0 =
 *     U(current) or U(current + dt/2));
 *   IBTK_LE_TRAPEZOIDAL:  X_new = (dt/2 * U0 + X_cur) + dt/2 * U1
 *     (IBMethod::trapezoidalStep, IBMethod.cpp:657-681: VecWAXPY then VecAXPY, U0 =
 *     U(current), U1 = U(new)).
 * Each step is a rounded multiply and a rounded add, as PETSc's loops compute it.
 * X_new may alias X_cur.  U1 is ignored (may be NULL) unless TRAPEZOIDAL. */
enum { IBTK_LE_EULER = 0, IBTK_LE_MIDPOINT = 1, IBTK_LE_TRAPEZOIDAL = 2 };
int ibtk_le_position_update(ibtk_le_ctx ctx, int scheme, long long n, double dt, const double* X_cur_dev,
                            const double* U0_dev, const double* U1_dev, double* X_new_dev);

/* ---- Lagrangian force generation (IBStandardForceGen) ------------------------------
 * The F handed to spread: the sum of spring, beam and target-point forces
 * IBStandardForceGen::computeLagrangianForce (IBStandardForceGen.cpp:265-313) computes
 * from X and U between the position update and the spread.  The reference zeroes a
 * scratch vector F_ghost, adds the springs (:778-892), the beams (:990-1099) and the
 * target points (:1150-1216) into it, each in a serial loop over k, and then adds
 * F_ghost to F.  At positions x = X + dX (dX: the nodes' periodic displacements, :289):
 *   spring k (master m, slave s, kappa, L):  D = x[s] - x[m], R = sqrt(D.D) summed left
 *     to right, skipped when R < DBL_EPSILON; f = ((kappa (R - L)) / R) D;
 *     F[m] += f, F[s] -= f      (the default law, IBSpringForceFunctions.h:117-120)
 *   beam k (master m, next, prev, K, C):     f = K (((x[next] + x[prev]) - 2 x[m]) - C);
 *     F[m] += 2 f, F[next] -= f, F[prev] -= f
 *   target point k (node i, K, E, X0):       F[i] += K (X0 - x[i]) - E U[i]
 * The plan keeps, per node, the list of its contributions in that order (springs by k,
 * then beams by k -- master, next, prev within one k --, then target points by k), and
 * one gather kernel, a lane per node, evaluates every contribution from the reference's
 * operands with the reference's operations and sums them in list order: no atomics, the
 * serial loops' result bit for bit.  A node with a very long list runs serially in its
 * lane.
 *
 * The set_* calls take HOST arrays of NODE indices in [0, n_nodes) -- the vectors
 * IBStandardForceGen caches in d_spring_data / d_beam_data / d_target_point_data before
 * its multiply by NDIM (petsc_*_node_idxs / NDIM) --, validate them
 * (IBTK_LE_ERR_ARG: an index out of range, mastr == slave / next / prev, which the
 * reference asserts against, a negative count, a NULL fg, a non-zero spring force
 * function index: only the default Hookean law runs on the device, registered host
 * function pointers do not) and replace that class of the plan (n = 0 clears it); they
 * block until the plan is on the device.  A failed call leaves the plan as it was.  Row
 * offsets are 64-bit, so no count an int can hold overflows them (IBTK_LE_ERR_RANGE is
 * never needed).  n_nodes may include trailing ghost nodes; the library does not
 * distinguish them.  fcn_idx, curv and eta may be NULL (all zero). */
typedef struct ibtk_le_forcegen_s* ibtk_le_forcegen;
int ibtk_le_forcegen_create(ibtk_le_ctx ctx, int ndim, int n_nodes, ibtk_le_forcegen* out);
int ibtk_le_forcegen_destroy(ibtk_le_forcegen fg);
int ibtk_le_forcegen_set_springs(ibtk_le_forcegen fg, int n, const int* mastr, const int* slave, const double* kappa,
                                 const double* rest, const int* fcn_idx);
int ibtk_le_forcegen_set_beams(ibtk_le_forcegen fg, int n, const int* mastr, const int* next, const int* prev,
                               const double* bend, const double* curv);
int ibtk_le_forcegen_set_targets(ibtk_le_forcegen fg, int n, const int* node, const double* kappa, const double* eta,
                                 const double* X0);
/* F = F + acc (accumulate != 0) or F = acc on [n_nodes][ndim] device arrays, ordered on
 * the context stream: no host synchronisation, no allocation.  dX_dev may be NULL (zero
 * displacements); U_dev may be NULL (read as zero) unless some target point has
 * eta != 0.  With nothing set, F is left untouched when accumulating and zeroed
 * otherwise.  F must not alias X, dX or U. */
int ibtk_le_forcegen_compute(ibtk_le_ctx ctx, ibtk_le_forcegen fg, const double* X_dev, const double* dX_dev,
                             const double* U_dev, double* F_dev, int accumulate);

/* ---- The force plan rebuilt on the device when the nodes are renumbered ---------------
 * LDataManager::endDataRedistribution gives the nodes new local indices at every regrid;
 * the reference then runs IBStandardForceGen::initializeLevelData again, which renumbers
 * the specs ("master by master in local node order, deck order within a master") and so
 * changes every node's summation order.  ibtk_le_forcegen_set_* would rebuild the plan on
 * the host and upload it; the calls below keep the specs on the device in LAGRANGIAN
 * vertex indices and deck order (uploaded once per structure set) and rebuild the plan
 * from them with device work alone.
 *
 * ibtk_le_forcespecs: the store, over num_vertex Lagrangian vertices.  The set_* calls
 * take HOST arrays in deck order with what does not depend on the numbering settled by
 * the caller: a spring's master is its smaller Lagrangian index and a repeated edge has
 * the parameters of its first line on every line (IBStandardInitializer.cpp:979-987,
 * 2848; ibamr_amd.forcegen.ForceSpecs.lagrangian_arrays does both); a target point
 * carries its anchor X0[k][ndim] inline.  They validate on the host before any device
 * call (IBTK_LE_ERR_ARG with a message: a NULL store, a negative count, a NULL array with
 * n > 0, an index outside [0, num_vertex), mastr == slave / next / prev, fcn_idx != 0)
 * and then replace that class of the store with a blocking upload (n = 0 clears it).
 * fcn_idx, curv and eta may be NULL.  ctx may be NULL: such a store only validates -- a
 * set_* with valid arguments and n > 0 then returns IBTK_LE_ERR_ARG ("without a
 * context") -- and cannot be renumbered from. */
typedef struct ibtk_le_forcespecs_s* ibtk_le_forcespecs;
int ibtk_le_forcespecs_create(ibtk_le_ctx ctx, int ndim, int num_vertex, ibtk_le_forcespecs* out);
int ibtk_le_forcespecs_destroy(ibtk_le_forcespecs fs);
int ibtk_le_forcespecs_set_springs(ibtk_le_forcespecs fs, int n, const int* mastr, const int* slave,
                                   const double* kappa, const double* rest, const int* fcn_idx);
int ibtk_le_forcespecs_set_beams(ibtk_le_forcespecs fs, int n, const int* mastr, const int* next, const int* prev,
                                 const double* bend, const double* curv);
int ibtk_le_forcespecs_set_targets(ibtk_le_forcespecs fs, int n, const int* node, const double* kappa,
                                   const double* eta, const double* X0);
/* Replaces all three classes of fg's plan with the plan of the numbering order_dev:
 * order_dev[i] (device, n_order <= n_nodes ints) is the Lagrangian index of node i --
 * what ibtk_le_node_distribution returns, trailing ghost nodes included if the caller has
 * them.  The result is byte for byte what ibtk_le_forcegen_set_* build for perm =
 * inverse(order): the same 64-bit row offsets and the same records in the same order
 * (springs ascending in the new k, the rank in a stable sort of the deck by perm[master];
 * beams likewise with the roles master, next, prev within one k; target points in a
 * stable sort by perm[node]).  A class the store does not hold becomes empty.
 *
 * A vertex that order does not name is absent.  A spec whose master (target point: whose
 * vertex) is absent is dropped -- a rank holding part of the structures calls it this
 * way; a kept spec with an absent slave, next or prev is an error.
 *
 * order is not trusted: an entry outside [0, num_vertex) and a Lagrangian index named
 * twice are found by the kernel that inverts order, which range-checks every entry before
 * it uses it as an index, and a kept spec with an absent endpoint by the key kernels;
 * every later kernel skips what was flagged.  On any of the three the call returns
 * IBTK_LE_ERR_ARG with a message naming the first offending entry, vertex or spec, every
 * class of the plan is left empty and the plan invalid: ibtk_le_forcegen_compute (and the
 * plan read-back) return IBTK_LE_ERR_ARG until a renumber or a set_* succeeds.
 *
 * All work is ordered on ctx's stream and the call ends with one small device-to-host
 * read of the status record (it blocks; it is a regrid-time call, compute stays free of
 * host synchronisation).  Its buffers are sized from the store's totals on the first
 * call, after a wait for the stream; a later call with the same store allocates nothing.
 * More than 2^31 - 1 entries in a class (2 per spring, 3 per beam): IBTK_LE_ERR_RANGE.
 * compute needs U exactly when a KEPT target point has eta != 0. */
int ibtk_le_forcegen_renumber(ibtk_le_ctx ctx, ibtk_le_forcegen fg, ibtk_le_forcespecs fs, const int* order_dev,
                              int n_order);
/* out[0:3] the springs, beams and target points the last renumber kept, out[3:6] those it
 * dropped, out[6] the device bytes the plan and its renumber scratch hold, out[7] the
 * device allocations renumber has made for this plan so far. */
int ibtk_le_forcegen_renumber_stats(ibtk_le_forcegen fg, long long* out);
/* The plan read back, for tests and debugging.  cls: 0 springs, 1 beams, 2 target points.
 * *n_entries: 2 per spring, 3 per beam, 1 per target point.  plan_read copies the n_nodes
 * + 1 row offsets and the n_entries records (rec_bytes = n_entries * the record's size,
 * else IBTK_LE_ERR_ARG) to the host; it blocks.  Records, without padding:
 *   springs        {int m, s; double kappa, rest;}
 *   beams          {int m, next, prev, role; double bend, curv[ndim];}   role 0 / 1 / 2: the
 *                  row's node is the master / next / prev
 *   target points  {double kappa, eta, X0[ndim];} */
int ibtk_le_forcegen_plan_size(ibtk_le_forcegen fg, int cls, long long* n_entries);
int ibtk_le_forcegen_plan_read(ibtk_le_forcegen fg, int cls, long long* off_host, void* rec_host,
                               long long rec_bytes);

/* ---- The force Jacobian (the other half of IBLagrangianForceStrategy) -----------------
 * IBStandardForceGen::computeLagrangianForceJacobian (IBStandardForceGen.cpp:498-665) adds,
 * with MatSetValuesBlocked(ADD_VALUES), NDIM x NDIM blocks into a matrix over the nodes, in
 * three serial loops over k.  At positions x = X + dX, with the caller's X_coef and U_coef:
 *   spring k (m, s, kappa, L): D = x[s] - x[m]; R = D.norm(), Eigen 3.2.1's unrolled
 *     reduction sqrt(D0^2 + (D1^2 + D2^2)) in 3-D (Redux.h:77-106; not the force loop's
 *     left-to-right sum), sqrt(D0^2 + D1^2) in 2-D; T = kappa (R - L), dT_dR = kappa (the
 *     default law and its derivative, IBSpringForceFunctions.h:117-131);
 *       dF(i, j) = X_coef ((T / R) delta_ij + (((dT_dR - T / R) D[i]) D[j]) / (R R)).
 *     dF.data() is column-major and MatSetValuesBlocked reads it row-major, so the STORED
 *     element (r, c) of the block is dF(c, r) -- the two differ in the last bit, (a D[i]) D[j]
 *     does not commute under rounding.  Blocks (m, s) and (s, m) += dF; (m, m) and (s, s) +=
 *     dF * -1.0.  There is no guard for R = 0: a spring between coincident nodes puts NaN
 *     (0 / 0) into its four blocks, (m, s), (s, m), (m, m), (s, s), and nowhere else.
 *   beam k (m, next n, prev p, bend): diagonal blocks, the zeros off their diagonals added
 *     like every other element: (p,p) (p,n) (n,p) (n,n) += (-1.0 bend) X_coef; (p,m) (n,m)
 *     (m,p) (m,n) += (2.0 bend) X_coef; (m,m) += (-4.0 bend) X_coef.
 *   target point k (node i, K, E): (i,i) += diagonal ((-X_coef) K) - (U_coef E).
 *
 * ibtk_le_forcejac is that matrix on the device in block-CSR over the n_nodes of a force
 * generator: rowptr[n_nodes + 1] int64, col[n_blocks] int32 ascending within a row,
 * val[n_blocks][ndim][ndim] float64, row-major blocks.  The pattern is exactly the set of
 * blocks those calls touch plus the diagonal block of every node (which the reference
 * preallocates, :351); repeated entries -- a repeated edge, a spring and a beam between
 * the same nodes, a beam with next == prev -- are one block.
 *
 * create builds the pattern on the device from fg's CURRENT plan (a 64-bit radix sort of
 * the (row, col) keys of every plan entry, a scan; no host trip but one small read of the
 * block count, which blocks) and, per block, the plan entries that contribute to it in the
 * reference's order, so that assemble searches nothing.  ctx must be the context fg was
 * created with.  rebuild does it again
 * after fg was changed by a set_* or a renumber: every such call advances fg's plan
 * generation, and assemble and apply return IBTK_LE_ERR_ARG ("the pattern is stale ...
 * call ibtk_le_forcejac_rebuild") while J's pattern is of an older generation.  A plan left
 * invalid by a failed renumber is refused as ibtk_le_forcegen_compute refuses it.  The
 * arrays and the scratch are sized on the first build; a rebuild over a plan with the same
 * counts (nodes, springs, beams, blocks) allocates nothing.  More than 2^31 - 1 candidate
 * blocks (n_nodes + 2 springs + 9 beams): IBTK_LE_ERR_RANGE.  fg must outlive J.
 *
 * Contexts.  Every ibtk_le_forcejac_* call that takes a ctx wants the ONE context fg was
 * created with (another: IBTK_LE_ERR_ARG, "another context"): J's arrays are written by
 * rebuild and assemble and read by apply in the order of that context's stream, and nothing
 * else orders them.  ibtk_le_forcegen_linearized and ibtk_le_forcegen_jacobian_nnz below
 * only READ the plan, as ibtk_le_forcegen_compute does, and follow its rule: any context on
 * the plan's device (another device: IBTK_LE_ERR_ARG).  That is safe because whatever
 * changes a plan -- a set_* or a renumber -- returns only after the plan is in place. */
typedef struct ibtk_le_forcejac_s* ibtk_le_forcejac;
int ibtk_le_forcejac_create(ibtk_le_ctx ctx, ibtk_le_forcegen fg, ibtk_le_forcejac* out);
int ibtk_le_forcejac_destroy(ibtk_le_forcejac J);
int ibtk_le_forcejac_rebuild(ibtk_le_ctx ctx, ibtk_le_forcejac J);
/* val = the Jacobian at X + dX ([n_nodes][ndim] device arrays; dX_dev may be NULL; one
 * rounded add per use).  Every block starts at +0.0, as after MatZeroEntries, and takes its
 * contributions as whole blocks in the order of the reference's calls: springs ascending
 * in k, then beams ascending in k, then target points.  One lane owns each block: it sums
 * the block's contributions in registers, in the order the pattern build recorded for it
 * (the block's run of the row's plan entries; on a diagonal block the row's springs first,
 * the row's target points last), and stores the block once.  No floating-point atomics, the
 * same bits run to run, and bit for bit the serial assembly (signed zeros included; NaN for
 * coincident spring nodes, see above).  One rounded operation per reference operation, IEEE
 * sqrt and divide.  Ordered on ctx's stream, no host synchronisation, no allocation. */
int ibtk_le_forcejac_assemble(ibtk_le_ctx ctx, ibtk_le_forcejac J, const double* X_dev, const double* dX_dev,
                              double X_coef, double U_coef);
/* Y = Y + J V (accumulate != 0) or Y = J V with the assembled values; V and Y are
 * [n_nodes][ndim] float64 device arrays (8-byte alignment suffices), Y must not alias V.
 * The summation order is fixed by the pattern, so the result has the same bits run to run:
 * the doubles of block row i, in storage order, are numbered e = 0, 1, ...; with b = e /
 * ndim^2, r = (e % ndim^2) / ndim and c = e % ndim, lane l of 16 adds the products val[e]
 * V[col[b]][c] for e = l, l + 16, l + 32, ... in that order to its partial sum of
 * component r (from +0.0), and the 16 partial sums of a component are combined pairwise
 * at lane distances 8, 4, 2, 1.  No host synchronisation, no allocation. */
int ibtk_le_forcejac_apply(ibtk_le_ctx ctx, ibtk_le_forcejac J, const double* V_dev, double* Y_dev, int accumulate);
/* The block count and the DEVICE pointers of rowptr, col and val (any may be NULL), to wrap
 * or to copy into a block AIJ matrix; they stay valid until the next rebuild or destroy. */
int ibtk_le_forcejac_pattern(ibtk_le_forcejac J, long long* n_blocks, const long long** rowptr_dev,
                             const int** col_dev, double** val_dev);
/* The same to the host, for tests and debugging; it blocks.  n_blocks must be the pattern's
 * count; val_host may be NULL (pattern only), else the values must have been assembled. */
int ibtk_le_forcejac_read(ibtk_le_forcejac J, long long* rowptr_host, int* col_host, double* val_host,
                          long long n_blocks);
/* out[0] blocks, out[1] candidate blocks (n_nodes + 2 springs + 9 beams), out[2] the device
 * bytes J holds, out[3] the device allocations its builds have made so far, out[4] its
 * builds, out[5] 1 if the pattern is of fg's current plan generation. */
int ibtk_le_forcejac_stats(ibtk_le_forcejac J, long long* out);
/* Y (+)= J(X + dX) V without a matrix: the exact product in place of the MatMFFD
 * difference of IBMethod::computeLinearizedLagrangianForce (IBMethod.cpp:710-723).  The
 * gather kernel of compute with every contribution's block formed exactly as assemble forms
 * it and applied to V at the block's column at once -- row by row of the block, left to
 * right -- in contribution order: a node's springs by k (the off-diagonal block, then the
 * diagonal one), its beams by k (columns prev, next, master), its target points.  Same bits
 * run to run.  Arguments as compute's; Y must not alias X, dX or V. */
int ibtk_le_forcegen_linearized(ibtk_le_ctx ctx, ibtk_le_forcegen fg, const double* X_dev, const double* dX_dev,
                                const double* V_dev, double X_coef, double U_coef, double* Y_dev, int accumulate);
/* The per-block-row counts of computeLagrangianForceJacobianNonzeroStructure (:315-496)
 * before its expansion to scalar rows: d_nnz = 1 and o_nnz = 0, each spring adds 1 at its
 * master and at its slave (to d_nnz if the SLAVE is local, else to o_nnz), each beam the
 * weights of the reference's four cases (:401-455), its deliberate over-count included.  A
 * node is local iff its index is < n_local (0 <= n_local <= n_nodes: trailing ghost nodes).
 * Both outputs are n_nodes int32 on the device.  No host synchronisation. */
int ibtk_le_forcegen_jacobian_nnz(ibtk_le_ctx ctx, ibtk_le_forcegen fg, int n_local, int* d_nnz_dev,
                                  int* o_nnz_dev);

/* ---- Kirchhoff rods (IBKirchhoffRodForceGen, GeneralizedIBMethod) ---------------------
 * The Lagrangian side of the generalized IB step, 3-D and fp64: the force F and torque N
 * of IBKirchhoffRodForceGen::computeLagrangianForceAndTorque (IBKirchhoffRodForceGen.cpp:
 * 326-527) from the positions X and the director triads D ([n_nodes][9], rows D1 D2 D3),
 * and the rotation of the triads by the interpolated angular velocity
 * (GeneralizedIBMethod::eulerStep / trapezoidalStep, GeneralizedIBMethod.cpp:326-447).
 * W and N themselves travel through ibtk_le_interp / ibtk_le_spread as depth-3 data.
 *
 * Rod k (curr, next, ds a1 a2 a3 b1 b2 b3 kappa1 kappa2 tau), :401-469:
 *   A = sum_i D_i[next] D_i[curr]^T,  D_i_half = sqrt(A) D_i[curr]  (the principal root)
 *   dX = X[next] - X[curr]
 *   F_half = b1 (D1_half . dX/ds) D1_half + b2 (D2_half . dX/ds) D2_half
 *            + b3 (D3_half . dX/ds - 1) D3_half
 *   N_half = a1 ((D2[next] - D2[curr])/ds . D3_half - kappa1) D1_half
 *            + a2 ((D3[next] - D3[curr])/ds . D1_half - kappa2) D2_half
 *            + a3 ((D1[next] - D1[curr])/ds . D2_half - tau) D3_half
 *   F[curr] += F_half,  N[curr] += N_half + 0.5 dX x F_half
 *   F[next] -= F_half,  N[next] += -N_half + 0.5 dX x F_half
 * The reference adds all curr contributions in ascending k and then all next contributions
 * in ascending k (two VecSetValuesBlocked(ADD_VALUES) calls per vector, :489-515).  The
 * plan keeps that list per node -- one CSR over the nodes with 64-bit row offsets, two
 * entries per rod, a node's curr-role entries in ascending k and then its next-role
 * entries in ascending k, every entry the whole rod {int curr, next; double p[10];} (88
 * bytes, no padding; the row's node is the curr end when record.curr == node) -- and one
 * kernel, a lane per node, evaluates every rod of its row and sums in list order: no
 * atomics, bit-stable run to run, and the two ends of a rod see the identical F_half and
 * N_half.
 *
 * The principal square root is computed for a general 3x3 matrix (the triads drift; A is
 * not assumed to be a rotation) by a Denman-Beavers iteration capped at a compile-time
 * count; sqrt(I) is I exactly.  The reference takes Eigen's Schur-based root: the results
 * agree to rounding, not bit for bit.  An A with an eigenvalue on the closed negative real
 * axis (neighbouring triads half a turn apart) has no principal root and the reference's
 * result there is unspecified: F and N of the two nodes of such a rod may be anything,
 * NaN included; no other node is affected.
 *
 * set_rods takes HOST arrays of NODE indices in [0, n_nodes) and params[n][10], in the
 * reference's order (ibamr_amd.rods.RodSpecs.arrays), validates them on the host before
 * any device call (IBTK_LE_ERR_ARG with a message: a NULL handle, n < 0, a NULL array with
 * n > 0, an index out of range, curr == next, a non-finite parameter; ds == 0 is accepted
 * as the reference accepts it -- it divides by it and the result is inf or NaN), builds
 * the plan with a stable counting sort and replaces the plan with a blocking upload (n = 0
 * clears it).  A failed call leaves the plan as it was (the new plan goes into fresh device
 * buffers that replace the old ones once it is uploaded).  A handle created with ctx NULL
 * only validates: a set_rods with valid arguments and n > 0 then returns IBTK_LE_ERR_ARG
 * ("without a context").
 *
 * compute: F = F + acc (accumulate_F != 0) or F = acc, likewise N, on [n_nodes][3] device
 * arrays, ordered on the context stream: no allocation, no host synchronisation.  (The
 * reference adds to the F the standard generator left and zeroes N first,
 * GeneralizedIBMethod.cpp:488.)  With no rods set, F and N are left untouched when
 * accumulating and zeroed otherwise.  F and N must not overlap each other, X or D.  ctx must
 * be the context the handle was created with (IBTK_LE_ERR_ARG otherwise): set_rods and
 * destroy wait for that context's stream before they release the plan's buffers. */
typedef struct ibtk_le_rodgen_s* ibtk_le_rodgen;
int ibtk_le_rodgen_create(ibtk_le_ctx ctx, int n_nodes, ibtk_le_rodgen* out);
int ibtk_le_rodgen_destroy(ibtk_le_rodgen rg);
int ibtk_le_rodgen_set_rods(ibtk_le_rodgen rg, int n, const int* curr, const int* next, const double* params);
int ibtk_le_rodgen_compute(ibtk_le_ctx ctx, ibtk_le_rodgen rg, const double* X_dev, const double* D_dev,
                           double* F_dev, double* N_dev, int accumulate_F, int accumulate_N);
/* The plan read back, for tests and debugging: *n_entries = 2 per rod; plan_read copies the
 * n_nodes + 1 row offsets and the records (rec_bytes = n_entries * 88, else
 * IBTK_LE_ERR_ARG) to the host; it blocks. */
int ibtk_le_rodgen_plan_size(ibtk_le_rodgen rg, long long* n_entries);
int ibtk_le_rodgen_plan_read(ibtk_le_rodgen rg, long long* off_host, void* rec_host, long long rec_bytes);
/* The director update over n nodes: e = W0 (IBTK_LE_EULER) or 0.5 (W0 + W1)
 * (IBTK_LE_TRAPEZOIDAL; W1 is ignored and may be NULL otherwise), [n][3] each.  Where
 * |e| > DBL_EPSILON the three rows of D ([n][9]) are rotated by the Rodrigues matrix of
 * GeneralizedIBMethod.cpp:357-361 with theta = |e| dt and e /= |e|; elsewhere they are
 * copied bit for bit.  IBTK_LE_MIDPOINT returns IBTK_LE_ERR_ARG, as the reference refuses
 * it (:383-389).  D_new may be D_cur itself; any other overlap of D_new with D_cur, W0 or
 * W1 is IBTK_LE_ERR_ARG.  Ordered on the context stream, no host synchronisation. */
int ibtk_le_director_update(ibtk_le_ctx ctx, int scheme, long long n, double dt, const double* D_cur_dev,
                            const double* W0_dev, const double* W1_dev, double* D_new_dev);

/* ---- IMPMethod: the immersed material point method ------------------------------------
 * The four device stages of src/IB/IMPMethod.cpp for one patch of side-centred data, 2-D and
 * 3-D.  IMPMethod carries its own IB_6 kernel with its derivative (:119-171): the same NINT
 * anchor and six points as "IB_6", but the powers of r are running products (r3 = r r2, ...)
 * where the Fortran kernels use binary powering, so its weights are not ibtk_le_interp's to
 * the last bit.  The component frame is the reference's: x_lower[d] - 0.5 dx[d] and iupper[d]
 * + 1 for d == component.
 *
 * m: markers binned with kernel IB_6 on `geom` (ibtk_le_markers_bin; list entries, indices,
 * Xshift and duplicates as in ibtk_le_interp), not a level and not a fixed-capacity list.
 * geom->gcw[d] >= 4 in every dim (IBTK_LE_ERR_GHOST_WIDTH otherwise).  Positions are the
 * binned ones, X(s) + Xshift(l).  DEVIATION: the reference evaluates its kernel at X(s) and
 * ignores the periodic offset of an image node; with Xshift = 0 the two agree.
 *
 * ibtk_le_imp_interp (IMPMethod::interpolateVelocity :460-536): U_dev[s][NDIM] and
 * GradU_dev[s][NDIM * i + j] = d u_i / d x_j, from the stencil box clipped to the
 * component's ghost box, summed with dimension 0 fastest, w = (phi0 phi1) phi2,
 * U(c) += u w, dw_k = ((a_0) a_1) a_2 with a_d = dphi[d] / dx[d] for d == k and phi[d]
 * otherwise, Grad_U(c, k) -= u dw_k: bit for bit the reference's values.  Rows the list does
 * not name are not written; of duplicate entries the last one writes.  One launch (the first
 * interp after a binning with an index list also builds the duplicate table, which
 * synchronises, as ibtk_le_interp does).
 *
 * ibtk_le_imp_spread (::spreadForce :848-921): f(i_s) += (sum_k tau(c,k) dw_k) wgt / dV_c,
 * dV_c = (dx0 dx1) dx2, tau_dev[s][NDIM * c + k], wgt_dev[s].  clip = IBTK_LE_IMP_CLIP_PATCH
 * is the reference: the stencil is cut to toSideBox(patch_box, c), periodic images arrive
 * as list entries (ibtk_le_periodic_index_list); IBTK_LE_IMP_CLIP_GHOST cuts to the arrays'
 * ghost boxes, for a caller who then folds (ibtk_le_fold_periodic_ghosts) or applies
 * ibtk_le_phys_bdry_side(adjoint).  Nothing outside the clip boxes is written.  No atomics:
 * every point sums its contributions itself, in a fixed order (by anchor cell, list order
 * within a cell), so the result is bit-identical from run to run; it differs from the
 * reference's by that order and by f (wgt / dV) for (f wgt) / dV.  Four launches and a device
 * sort on the context stream, no host synchronisation.
 *
 * ibtk_le_imp_deformation_update (eulerStep, midpointStep, trapezoidalStep :547-716), rows
 * of NDIM^2 doubles: F_new = inv(I - dt/2 Gb)(I + dt/2 G0) F_cur with Gb = G0 (EULER: Grad U
 * at the current time; MIDPOINT: at the half time) or G1 (TRAPEZOIDAL: G0 current, G1 new;
 * G1 NULL is IBTK_LE_ERR_ARG).  EULER also writes F_half (dt/4 for dt/2) unless F_half_dev
 * is NULL; with another scheme a non-NULL F_half_dev is IBTK_LE_ERR_ARG.  tensor_inverse is
 * the cofactor form of ibtk/libmesh_utilities.h:310-339, in 2-D its 2x2 branch with
 * F(2,2) = 1.  F_new may be F_cur.
 *
 * ibtk_le_imp_stress: tau = PP FF^T (IMPMethod::computeLagrangianForce :756-764) with the
 * law of examples/IMP/explicit/ex0/main.cpp:68-89, PP = 2 c1 FF, - 2 p0 FF^-T when p0 != 0,
 * + beta log(det(FF^T FF)) FF^-T when beta != 0.  table_dev NULL: the scalars c1, p0, beta;
 * else point i takes row subdomain_dev[i] (int32) of table_dev[nsub][3] = {c1, p0, beta}
 * and the scalars are ignored (a row outside [0, nsub) gives that point a NaN stress).  The
 * reference's registered PK1 function is a host pointer; here tau is a device array, so a
 * caller may fill it by other means.
 *
 * The update and the stress validate before they need the context, so a NULL ctx with valid
 * arguments returns IBTK_LE_ERR_ARG ("null context"). */
enum { IBTK_LE_IMP_CLIP_PATCH = 0, IBTK_LE_IMP_CLIP_GHOST = 1 };
int ibtk_le_imp_interp(ibtk_le_ctx ctx, ibtk_le_markers m, const ibtk_le_patch_geom* geom, const double* const* u_dev,
                       double* U_dev, double* GradU_dev, const double* X_dev);
int ibtk_le_imp_spread(ibtk_le_ctx ctx, ibtk_le_markers m, const ibtk_le_patch_geom* geom, double* const* f_dev,
                       const double* tau_dev, const double* wgt_dev, const double* X_dev, int clip);
int ibtk_le_imp_deformation_update(ibtk_le_ctx ctx, int ndim, int scheme, long long n, double dt,
                                   const double* F_cur_dev, const double* G0_dev, const double* G1_dev,
                                   double* F_new_dev, double* F_half_dev);
int ibtk_le_imp_stress(ibtk_le_ctx ctx, int ndim, long long n, const double* F_dev, double* tau_dev, double c1, double p0,
                       double beta, const double* table_dev, int nsub, const int* subdomain_dev);

/* ---- Fluid sources and sinks ---------------------------------------------------------------
 * IBMethod::spreadFluidSource (src/IB/IBMethod.cpp:789-943) and ::interpolatePressure
 * (:945-1069) with IBStandardSourceGen::getSourceLocations behind them
 * (src/IB/IBStandardSourceGen.cpp:195-250), for one patch of cell-centred data of depth 1 laid
 * out by geom (ghosts; pitch in 3-D), 2-D and 3-D.  These loops are not LEInteractor calls:
 * the kernel function is cos_kernel(x, r) = 0.5 (1 + cos(pi x / r)) / r for |x| <= r, else 0
 * (:124-134), per source n and dimension d with (:832-845)
 *   R = max(floor(r_src[n] / dx[d] + 0.5), 2),  r = R dx[d],
 *   centre cell by IndexUtilities::getCellIndex of X_src[n] in the patch frame,
 *   half width int(r / dx[d]) + 1 (R for some spacings, R + 1 for others),
 * and the stencil box cut to the patch box, never to the ghost box (:848).  A weight is
 * w_d = cos_kernel(X_center - X_src[n][d], r), X_center = x_lower[d] + dx[d] (double(i -
 * ilower[d]) + 0.5) (:854-855).  Each w_d is evaluated once per (source, dimension, cell
 * index) into a table of the plan's workspace; the spread and the pressure interpolation read
 * the same tables, so they are adjoint to rounding.  The tables hold R <= 16: a larger R
 * returns IBTK_LE_ERR_ARG before anything is written (checked on the host from r_src and
 * geom->dx).
 *
 * ibtk_le_sources_create takes HOST arrays: the radii r_src[n_src] (finite, > 0) and n_pts
 * pairs (node[k], source[k]) -- node k, a local index in [0, n_nodes), carries source
 * source[k] in [0, n_src), the IBSourceSpec of the reference's LNode; a node named twice is an
 * error -- groups the nodes by source, each group in ascending local index, uploads the plan
 * (blocking) and allocates every workspace the device calls use.  The device calls below
 * run on the context stream, never synchronise with the host and allocate nothing.  ctx must
 * be the plan's context.  destroy waits for that stream.
 *
 * ibtk_le_source_locations (getSourceLocations :213-230): X_src_dev[NDIM k + d] = sum_i
 * X_dev[NDIM node_i + d] / double(count_k) over the nodes of source k in ascending local
 * index, from 0, every quotient rounded before it is added, one lane per (k, d): bit for bit
 * the reference's value on one rank.  A source without nodes gets 0.
 *
 * ibtk_le_source_spread (:828-859): q(i) += Q_src[n] wgt over the clipped box, wgt = (w0 w1)
 * w2 (w0 w1 in 2-D); a cell reached by several sources adds them in ascending n.  A cell is
 * owned by the lowest-numbered source whose clipped box holds it; the owner's lane adds every
 * covering contribution in that order and stores once.  No atomics; bit-stable from run to
 * run; nothing outside the union of the clipped boxes is written.  Two launches.
 *
 * ibtk_le_source_normalize (:863-941), totals_dev = {q_total, Q_sum, q_norm, integral_after}:
 * q_total = sum q dV over the patch box, dV = (dx0 dx1) dx2, by a fixed-order two-stage
 * reduction; Q_sum = sum_n Q_src[n] serially.  When |q_total - Q_sum| > 1e-12 and |q_total -
 * Q_sum| / max(max_n |Q_src[n]|, 1) > 1e-12 (:877) the call does not abort as the reference
 * does: it latches device flag 32, which ibtk_le_ctx_synchronize reports as
 * IBTK_LE_ERR_INVARIANT.  With normalize != 0 (dom_lo / dom_hi, HOST, the domain box):
 * q_norm = -q_total / vol, vol = double(cells of domain \ interior) dx0 dx1 dx2, interior
 * the domain box shrunk by one cell in every dimension but the last; each such cell in the
 * patch box gets += q_norm; integral_after is the integral again, and |integral_after| >
 * 1e-10 max(1, max |q|) (:934) latches the same flag.  With normalize == 0, q is only read,
 * q_norm = 0 and integral_after = q_total.  Two launches, or four.
 *
 * ibtk_le_source_pressure (:1005-1063): P_src_dev[n] = sum p(i) wgt - p_norm over the same
 * clipped box, wgt = ((w0 dx0) (w1 dx1)) (w2 dx2), one workgroup per source, every lane a
 * fixed share of the cells, then a fixed tree.  p_norm (:960-1003) = (sum p dV over the cells
 * of domain \ interior in the patch box) / (their number times dV) -- the reference adds dV
 * cell by cell, which differs in the last bits --; dom_lo and dom_hi both NULL: p_norm = 0.
 *
 * IBTK_LE_ERR_ARG before any device call: a null context, plan, geometry or array; ndim not 2
 * or 3; a geometry whose ndim is not the plan's; a dx that is not finite and positive;
 * exactly one of dom_lo / dom_hi, or an empty domain box; a node or source index out of
 * range.  n_src == 0 and an empty patch box are IBTK_LE_OK and write nothing.  One patch: the
 * reference's sums of X_src and P_src over ranks and patches, periodic images of a source
 * (it has none: a stencil ends at the patch box) and source strategies other than the
 * standard one are not here. */
typedef struct ibtk_le_sources_s* ibtk_le_sources;
int ibtk_le_sources_create(ibtk_le_ctx ctx, int ndim, int n_nodes, int n_src, const double* r_src, int n_pts,
                           const int* node, const int* source, ibtk_le_sources* out);
int ibtk_le_sources_destroy(ibtk_le_sources s);
int ibtk_le_source_locations(ibtk_le_ctx ctx, ibtk_le_sources s, const double* X_dev, double* X_src_dev);
int ibtk_le_source_spread(ibtk_le_ctx ctx, ibtk_le_sources s, const ibtk_le_patch_geom* geom, double* q_dev,
                          const double* X_src_dev, const double* Q_src_dev);
int ibtk_le_source_normalize(ibtk_le_ctx ctx, ibtk_le_sources s, const ibtk_le_patch_geom* geom, double* q_dev,
                             const int* dom_lo, const int* dom_hi, const double* Q_src_dev, int normalize,
                             double* totals_dev);
int ibtk_le_source_pressure(ibtk_le_ctx ctx, ibtk_le_sources s, const ibtk_le_patch_geom* geom, const double* p_dev,
                            const double* X_src_dev, double* P_src_dev, const int* dom_lo, const int* dom_hi);

/* ---- Flow meters and pressure gauges ---------------------------------------------------------
 * IBInstrumentPanel (src/IB/IBInstrumentPanel.cpp) for one 3-D patch of side-centred u and
 * cell-centred p of depth 1 laid out by geom (ghosts; pitch), on one rank:
 * initializeHierarchyDependentData (:698-923) with init_meter_elements (:133-194), and
 * readInstrumentData (:925-1182) with linear_interp (:315-501) and compute_flow_correction
 * (:199-234).  A 2-D geometry returns IBTK_LE_ERR_ARG: the reference aborts there (:121-127).
 * The arithmetic is + - * /, sqrt, ceil and floor, written operation for operation with the
 * associations of the reference's Eigen 3.2.1 expressions (a fixed-size reduction is unrolled
 * as halves, Eigen/src/Core/Redux.h:77-106: a.dot(b) = a0 b0 + (a1 b1 + a2 b2), norm = sqrt(x^2
 * + (y^2 + z^2)); v / s divides, v /= s multiplies by 1 / s), so every output is the reference's one-rank value bit for bit (a NaN is a
 * NaN: its sign and payload are the processor's).
 *
 * ibtk_le_meters_create takes HOST arrays: n_pts triples (node[k], meter[k], meter_node[k]) --
 * local node node[k] in [0, n_nodes) is perimeter node meter_node[k] of meter meter[k] in [0,
 * n_meters), the IBInstrumentationSpec of the reference's LNode.  P_l = 1 + the largest node
 * index of meter l (:589-625).  IBTK_LE_ERR_ARG: an index out of range, a local node named
 * twice, a (meter, node index) pair named twice or missing, max_web_nodes odd or < 2.
 * max_web_nodes is the capacity of a web in the radial direction: its size follows the
 * device-resident X, so the host cannot size it; the workspace holds sum_l P_l max_web_nodes
 * web patches, and P_l max_web_nodes <= 4096 for every meter (IBTK_LE_ERR_ARG beyond: a
 * meter's sort keys fill 32 KiB of LDS).  create uploads the plan (blocking) and allocates every
 * workspace; update and read are one launch each on the context stream, never synchronise
 * with the host and allocate nothing.  ctx must be the plan's context.  destroy waits for that
 * stream.  n_meters == 0 is IBTK_LE_OK and every later call writes nothing; so is an empty box.
 *
 * ibtk_le_meters_update, for one level that is one patch: X_perimeter[l][n] = X_dev[3 node];
 * X_centroid[l] the serial sum over n from 0, each component then multiplied by 1.0 /
 * double(P_l) (:784-792: Eigen's v /= s multiplies by Scalar(1) / s, SelfCwiseBinaryOp.h:181-193); r_max[l] = max_n norm(X_perimeter - X_centroid) (:795-803); nw_l = 2
 * int(ceil(r_max / h_finest)) (:828); the web centroids X_web[l][m][n] and area vectors
 * dA_web[l][m][n], m < P_l, n < nw_l (:133-194).  Each web patch and each meter centroid gets
 * its cell by IndexUtilities::getCellIndex in the domain frame (dom_lo, dom_hi, dom_xlo,
 * dom_xup: HOST, 3 each) with geom->dx (:881-882, :903-904), and is counted iff that cell lies
 * in the patch box (:889, :911); nothing periodic is applied and an uncounted web patch is
 * dropped silently, as in the reference.  nw_l > max_web_nodes (or an r_max / h_finest no int
 * holds) latches device flag 64, which ibtk_le_ctx_synchronize reports as
 * IBTK_LE_ERR_INVARIANT: that meter's values are NaN until an update fits it, the other meters
 * are unaffected.  r_max == 0 gives nw = 0: flow 0 - correction, mean pressure 0 / 0, point
 * pressure as usual.
 *
 * ibtk_le_meters_read: values_dev[3 l + {0, 1, 2}] = {flow, mean pressure, point pressure} of
 * meter l from u_dev[3] (side, the arrays of the three axes), p_dev (cell) and the marker
 * velocities U_dev[3 node + d], with the box of the last update.  For a counted web patch in
 * cell i, X_cell[d] = x_lower[d] + dx[d] (double(i_d - ilower[d]) + 0.5) (:990-996); the side
 * rule (:434-501) shifts 0..1 along the axis and -1..0 or 0..1 across it by X[d] < X_cell[d],
 * X_side carries the -0.5 dx offset on the axis, and the lower side of cell i + shift is read;
 * the cell rule is :315-369; in both wgt = (w0 w1) w2, w_d = (X[d] < Xc[d] ? X[d] - (Xc[d] -
 * dx[d]) : (Xc[d] + dx[d]) - X[d]) / dx[d], i2 outermost and i0 innermost, U += v wgt from 0.
 * Per meter flow += U . dA, mean += P norm(dA), A += norm(dA), mean /= A (:1073); the point
 * pressure is the cell rule at the centroid if the centroid is counted, else 0 (:1056); the
 * correction (:199-234, :1142-1156) is subtracted from the flow.  The three sums are serial
 * from +0.0 in the reference's order: the cells of the patch box with x fastest and, within
 * a cell, the meter's web patches with m ascending, then n.  No floating-point atomics; the
 * same bits from run to run.  u_dev == NULL skips the flow sum (flow = 0 - correction), p_dev
 * == NULL both pressures (NaN and 0).  The rules read one ghost layer: a ghost width < 1 in
 * any dimension is IBTK_LE_ERR_GHOST_WIDTH.  A box other than the last update's, or a read
 * before any update, is IBTK_LE_ERR_ARG.
 *
 * ibtk_le_meters_workspace copies one array of the plan's workspace into dst_dev (device,
 * `count` elements, which must be the array's size) on the context stream.  With L meters, S
 * = sum P_l perimeter nodes and W = S max_web_nodes: X_CENTROID 3 L doubles; NUM_WEB_NODES L
 * ints (-1: not representable); X_WEB, DA_WEB 3 W doubles and CELL 3 W ints, COUNTED W ints
 * -- meter l's patches start at patch max_web_nodes (P_0 + ... + P_{l-1}), patch (m, n) the
 * (m nw_l + n)-th of them; a meter that latched flag 64 keeps what it held --; CENTROID_CELL
 * 4 L ints (the cell, then counted); X_PERIMETER 3 S doubles.
 *
 * Not here: more than one level or patch ("the finest level that contains the point" and the
 * sums over ranks), z-slabs, a cell-centred u, the Silo plot output, restart, and
 * d_total_flow_volume (one multiply-add for the caller). */
typedef struct ibtk_le_meters_s* ibtk_le_meters;
enum {
    IBTK_LE_METERS_X_CENTROID = 0,
    IBTK_LE_METERS_NUM_WEB_NODES = 1,
    IBTK_LE_METERS_X_WEB = 2,
    IBTK_LE_METERS_DA_WEB = 3,
    IBTK_LE_METERS_CELL = 4,
    IBTK_LE_METERS_COUNTED = 5,
    IBTK_LE_METERS_CENTROID_CELL = 6,
    IBTK_LE_METERS_X_PERIMETER = 7
};
int ibtk_le_meters_create(ibtk_le_ctx ctx, int n_nodes, int n_meters, int n_pts, const int* node, const int* meter,
                          const int* meter_node, int max_web_nodes, ibtk_le_meters* out);
int ibtk_le_meters_destroy(ibtk_le_meters mt);
int ibtk_le_meters_update(ibtk_le_ctx ctx, ibtk_le_meters mt, const ibtk_le_patch_geom* geom, const int* dom_lo,
                          const int* dom_hi, const double* dom_xlo, const double* dom_xup, double h_finest,
                          const double* X_dev);
int ibtk_le_meters_read(ibtk_le_ctx ctx, ibtk_le_meters mt, const ibtk_le_patch_geom* geom, const double* const* u_dev,
                        const double* p_dev, const double* U_dev, double* values_dev);
int ibtk_le_meters_workspace(ibtk_le_ctx ctx, ibtk_le_meters mt, int which, void* dst_dev, long long count);

/* Position update fused with the z-slab migration classes (bench.py --move, ibamr_amd.slab.
 * migrate_device): X_new = the ibtk_le_position_update of (X_cur, U0, U1), wrapped
 * into [0, L) per dim as torch.remainder does; the markers' owners are the slabs of
 * their wrapped z cells (IndexUtilities::getCellIndex, LDataManager.cpp:1446; Nz
 * planes, nranks equal slabs).  order_dev (M ints) receives a stable partition of
 * the marker indices [staying | to rank-1 | to rank+1 | further], each part in
 * input order; counts_dev (4 ints, device) the part sizes.  Stream-ordered, no
 * host sync (the redistribution LDataManager.cpp:1504-1959 runs at regrid; SURVEY.md
 * 8(e) asks for it after every update).  X_new must not alias X_cur.  With two
 * ranks both neighbours are one rank: every leaver is in the second part. */
int ibtk_le_slab_update_partition(ibtk_le_ctx ctx, int scheme, long long M, double dt, const double* X_cur_dev,
                                  const double* U0_dev, const double* U1_dev, double* X_new_dev, const double* L,
                                  int Nz, int nranks, int rank, int* order_dev, int* counts_dev);
/* Fixed-capacity migration, no host sync (slab.update_and_migrate_fixed):
 * ibtk_le_slab_update_partition_count is the partition of the first *n_dev of
 * `capacity` rows; pack copies the down / up leavers of rows_dev ([capacity][depth]
 * doubles: X then the LData fields) into send buffers of send_cap rows each; after
 * the fixed-size exchange, unpack writes the stayers in order, then recv_counts[0]
 * rows of from_down and recv_counts[1] of from_up, into out_dev (out_cap rows) and
 * their number into *n_out_dev.  Leavers beyond send_cap, markers moving further
 * than one slab, or arrivals beyond out_cap raise device flag 8 (reported by
 * ibtk_le_ctx_synchronize): the caller sizes the buffers, the library never drops
 * a marker silently. */
int ibtk_le_slab_update_partition_count(ibtk_le_ctx ctx, int scheme, long long capacity, double dt,
                                        const double* X_cur_dev, const double* U0_dev, const double* U1_dev,
                                        double* X_new_dev, const double* L, int Nz, int nranks, int rank,
                                        const int* n_dev, int* order_dev, int* counts_dev);
int ibtk_le_slab_migrate_pack(ibtk_le_ctx ctx, const double* rows_dev, int depth, const int* order_dev,
                              const int* counts_dev, int send_cap, double* send_down_dev, double* send_up_dev);
int ibtk_le_slab_migrate_unpack(ibtk_le_ctx ctx, const double* rows_dev, int depth, const int* order_dev,
                                const int* counts_dev, const int* recv_counts_dev, const double* from_down_dev,
                                const double* from_up_dev, int send_cap, double* out_dev, int out_cap,
                                int* n_out_dev);

/* Diagnostics: masks_dev[c] (one byte per point of component c's ghosted array,
 * same layout) gets 1 at every point some listed stencil touches after clipping.
 * bench.py sums the masks for the exact algorithmic byte count |S_a|.
 * One mask pointer per component, packed whatever geom's pitch: NDIM for SIDE / EDGE,
 * q_depth for CELL / NODE (masks_dev[k]: depth k).  Limit: at most 4 components; more
 * returns IBTK_LE_ERR_ARG ("mark_stencils: at most 4 components"). */
int ibtk_le_mark_stencils(ibtk_le_ctx ctx, ibtk_le_markers m, int kernel, int centering, int axis,
                          const ibtk_le_patch_geom* geom, unsigned char* const* masks_dev, int q_depth,
                          const double* X_dev);

/* Diagnostics: number of device kernel launches issued by the last interp/spread/bin
 * call on this context, and the per-step timing of the last call's main kernel (ms,
 * measured with HIP events on the context stream when enabled). */
int ibtk_le_ctx_enable_timing(ibtk_le_ctx ctx, int enable);
/* Diagnostics: tuning overrides of the 3-D sweeps' work items (0 = default), both
 * taking effect at the next bin: "heavy" (own markers per item above which the
 * item is scheduled first; -1 never; default 4x the mean, at least 2048),
 * "seg_items" (target number of (column, segment)
 * items, which sets the segment length), "split_target" (own markers above
 * which a (column, segment) is cut into sub-segments), "min_piece" (planes per
 * sub-segment of a cut item, at least; default 8), "heavy_target" and
 * "heavy_min_piece" (the same for heavy items; defaults 2048 and 1), "strip" (column rows per
 * strip of the item order), "xcd_block" (light items over the XCDs in blocks of
 * this many table entries: 1 round-robin, -1 one range per XCD; default 8), and,
 * taking effect at the next spread, "f_stream" (1: the 3-D spread reads F at its marker row
 * through the candidate stream, which then carries each entry's row beside its sorted
 * position -- no gather pass and no sorted copy of F; -1: the gather pass into sorted
 * order, in line before the sweep; 0: the default, which is 1; bitwise the same result).
 * Any other key returns IBTK_LE_ERR_ARG.
 * Interp results do not depend on them; spread results are bit-stable for fixed
 * settings and may differ in the last bits between settings (same-point adds
 * within one 64-candidate chunk follow its step and lane order, and the chunk
 * boundaries move with the items). */
int ibtk_le_ctx_tune(ibtk_le_ctx ctx, const char* key, int value);
double ibtk_le_ctx_last_kernel_ms(ibtk_le_ctx ctx);
/* Counted 3-D spread sweeps (a diagnostic for the LDS-atomic bound; one host sync
 * per launch): while enabled, each spread call records the ds_add_f64 it issues,
 * out[0] = wave-instructions, out[1] = lane adds (summed over its components). */
int ibtk_le_ctx_count_adds(ibtk_le_ctx ctx, int enable);
int ibtk_le_ctx_last_adds(ibtk_le_ctx ctx, unsigned long long* out);

#ifdef __cplusplus
}
#endif
#endif /* IBTK_LE_H */
