/* glio_pgraph_cov.h -- the marginal covariance of EVERY node of the pose graph (glio_pgraph_*) from one factorisation, on the device: the 6 x 6
 * diagonal blocks of H^-1 and the blocks (i, i + 1), by a selected inversion (the Takahashi recurrence) over the nested dissection that
 * glio_pgraph_solve factors with -- backwards over the separator factor, then down every segment in parallel.
 * (A header of its own because the entry points and structs that glio_hip.h / glio_types.h / glio_pgraph_lm.h declare are pinned by the existing
 * ABI tests.)
 *
 * THE MATRIX.  H = J^T J of the graph at the CURRENT estimate: exactly the matrix glio_pgraph_marginal_covariance inverts.  Undamped, unregularised,
 * in the tangent frame of the retraction, rotation first.  diag[i] is the quantity the per-node call returns for node i (another elimination plan
 * there: the same to rounding, not to the bit).
 *
 * THE PLAN is the plan of a solve: node 0, the last node, every loop endpoint and a node after every segment_nodes interior nodes are separators; no
 * extra separator, no right-hand side.  The bits depend on the graph and on segment_nodes only.
 *
 * BITS.  Every sum is in a fixed order, no atomic takes part in a value.  Results are bit-identical from run to run; diag[i] is symmetric to the bit
 * (the lower triangle is computed and mirrored); next may be NULL without changing a bit of diag.
 *
 * NO SIDE EFFECT.  The call linearises at x as glio_pgraph_error does and factors in the solver's Y, seg and system workspaces, which every solve
 * fills anew: a glio_pgraph_solve / _solve_damped / _marginal_covariance / _error / _read_poses after it returns the bits it returns without it.
 * What the inversion needs beyond those is allocated at the first call: a graph that never asks allocates nothing.  ONE host wait, at the end; the
 * result goes through pinned memory and is handed over only if no pivot failed.  Not thread-safe against other calls on the same graph.
 *
 * REFUSALS.  GLIO_E_ARG: a null pg or diag (the _dev form: a null diag_dev); a graph without a node, or with neither a prior nor a GPS factor.
 * GLIO_E_NUMERIC: a pivot that is not positive and finite; bad_node names the node (of a separator pivot: the separator's node) met first in
 * elimination order, diag and next are untouched.  A refusal changes nothing another entry point reads. */
#ifndef GLIO_PGRAPH_COV_H_
#define GLIO_PGRAPH_COV_H_
#include "glio_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct glio_pgraph_cov_info {
    int32_t n_nodes, separators, full_row_separators, segment_nodes;   /* the plan that was used */
    int32_t bad_node;        /* -1, or the node (separator: its node) whose pivot was not positive and finite */
    int32_t pad_;
    double  min_pivot, max_pivot;   /* over the squared diagonal of the factor */
} glio_pgraph_cov_info;

/* sizeof() of glio_pgraph_cov_info; returns how many there are (1) */
int glio_pgraph_cov_struct_sizes(int32_t* out, int n);
/* diag [N][36]: block (i, i) of H^-1;  next [N-1][36] (may be NULL): block (i, i+1);  row major;  info may be NULL */
int glio_pgraph_covariance_all(glio_pgraph* pg, double* diag, double* next, glio_pgraph_cov_info* info);
/* the same arrays as device pointers, valid until the next call that changes the graph or asks again */
int glio_pgraph_covariance_all_dev(glio_pgraph* pg, const double** diag_dev, const double** next_dev, int* n_nodes);
/* device time of the last call from the start of the linearisation to the result's copy (HIP events), ms; GLIO_E_STATE before the first.
 * The copy moves what was asked: diag alone when next was NULL, nothing for the _dev form -- so this figure and the copy stage differ between the forms. */
int glio_pgraph_covariance_all_last_device_ms(glio_pgraph* pg, float* ms);
/* stages: linearise, segments + separator factor, separator inversion, segment down-sweep, copy */
int glio_pgraph_covariance_all_last_stage_ms(glio_pgraph* pg, float* ms5);

#ifdef __cplusplus
}
#endif
#endif /* GLIO_PGRAPH_COV_H_ */
