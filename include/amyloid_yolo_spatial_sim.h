/* amyloid_yolo_spatial_sim.h -- the second header of libamyloid_yolo_hip.so: random-labelling simulations for the spatial statistics
 * (wsi.spatial_envelope, wsi.quantify_region(spatial_envelope=...); csrc/ay_spatial.hip).
 *
 * Why a second header: the prototypes of include/amyloid_yolo.h are a frozen list (tests/golden/abi_sigs.json, AY_ABI_VERSION 2).
 * Entry points added after the freeze are declared here; they are exported by the same library, under the same conventions (status
 * codes, ay_last_error, ay_stream_t), and adding them breaks no caller of the first header.
 *
 * An observed K[a][b] says nothing without a null band.  Under RANDOM LABELLING the positions stay where they are and the class labels
 * are permuted among the counted rows; the band of K over many such labellings is what the observed value is held against.  Positions,
 * border distances, eligibility and the set of pairs within every radius are the same in every simulation -- only the class indices a
 * pair is booked under change -- so ONE pair walk serves all simulations.
 *
 * THE RELABEL RULE.  tests/spatial_envelope_reference.py restates it in NumPy (uint64 arrays) and in Python integers.
 *   The counted rows are THE PAIR RULE's (include/amyloid_yolo.h), with their observed classes and in row order: i_0 < ... < i_{N-1}
 *   with classes c_t.  n_c = the counted rows of class c, cum_c = n_0 + ... + n_{c-1}.
 *   A LABELLING gives every counted row a class.  Simulation 0 is the observed labelling.
 *   Simulation s >= 1 comes from 64-bit keys that are a pure function of (seed, s, t); all arithmetic modulo 2^64:
 *     z     = seed + s * 0x9E3779B97F4A7C15 + t * 0xD1B54A32D192ED03
 *     z     = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9
 *     z     = (z ^ (z >> 27)) * 0x94D049BB133111EB
 *     key_t = z ^ (z >> 31)
 *   rank_t = the position of t in the stable ascending order of the keys (ties go to the lower t).
 *   Row i_t gets the class c with cum_c <= rank_t < cum_{c+1}.
 *   This is a uniform permutation of the labels: every simulation keeps the class totals n_c.
 *   Known answers: seed = 0, s = 1, t = 0, 1 give 0xe220a8397b1dcdaf and 0x2d0f28c7e7e786b2; seed = 7, s = 3, t = 2 gives
 *   0xd3a8307ee11bd937; the stable argsort of the keys of seed = 0, s = 1, N = 8 is [7 3 1 2 5 4 6 0].
 *
 *   The device call takes the labellings as a TABLE and does not know where it came from: labels uint8 [n_rows][label_stride] on the
 *   device, row order, column s = simulation s, n_sims <= label_stride.  (wsi.relabel_table builds it on the host with NumPy, one
 *   stable argsort per simulation; column 0 is the observed labelling.)
 *   The counts of simulation s are THE PAIR RULE's (with a mask: THE PAIR WINDOW RULE's) with the class of every counted row i
 *   replaced by labels[i][s].  Positions, bd, eligibility and d2 are untouched: whether a row is counted is decided by its OBSERVED
 *   class, confidence and centre, as in THE PAIR RULE.
 *   A table value >= C on a counted row makes that row no centre, no partner and not `inside` in that simulation only, and sets the
 *   bit AY_PAIR_RELABEL_FLAG_LABEL in stats[2C + 2].  Table values of rows that are not counted are never read for a result.
 *   Output: sim_pairs int64 [S][C][C][B], sim_centres int32 [S][C][B], sim_inside int32 [S][C] (the counted rows labelled a in s with
 *     bd >= 0: stats[C + a] of that simulation); bd int32 [M] and stats int32 [2C + 3] as ay_pair_counts writes them, on the OBSERVED
 *     classes (stats[2C + 2] may also hold the bit above).  There is no nn: the nearest neighbour of a class changes with the labels.
 *   Integer sums only: a function of the inputs alone, the same bytes on every run and for every cell_side_q.
 *
 * ay_pair_counts_relabel: the contract of ay_pair_counts -- rows, mask, labels and every output on the device, radii_q and roi_q on the
 *   HOST; kernel launches only (no memset node, no allocation, no host read, no synchronisation), so the call can sit in a captured
 *   step; the call's own kernels reset every output; n_rows == 0 is legal (rows, labels, bd may then be NULL); no scratch.  mask ==
 *   NULL is THE PAIR RULE's rectangle (mask_cell is then ignored), otherwise THE PAIR WINDOW RULE with mask_cell.  Refused (-1,
 *   ay_last_error): null labels with n_rows > 0, n_sims outside 1 .. AY_PAIR_RELABEL_MAX_SIMS, label_stride < n_sims, and everything
 *   ay_pair_counts and ay_pair_counts_window refuse.  A label_stride that is a multiple of 64 makes the 64 labels of a row one
 *   aligned read.  workspace: 16-byte aligned, ay_pair_counts_relabel_workspace_bytes(...) bytes (0 for arguments the call
 *   refuses; mask_cell == 0 there means no mask). */
#ifndef AMYLOID_YOLO_SPATIAL_SIM_H
#define AMYLOID_YOLO_SPATIAL_SIM_H

#include "amyloid_yolo.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AY_PAIR_RELABEL_MAX_SIMS 1024
#define AY_PAIR_RELABEL_FLAG_LABEL 4

size_t ay_pair_counts_relabel_workspace_bytes(int n_rows, int num_classes, int n_radii, int slide_h, int slide_w, int r_max_q,
                                              int cell_side_q, int mask_cell /* 0: no mask */, int n_sims);
int ay_pair_counts_relabel(const float* rows, int n_rows, int num_classes, int slide_h, int slide_w, float min_conf,
                           const int32_t* radii_q, int n_radii, const int32_t* roi_q, int border, int cell_side_q,
                           const uint8_t* mask /* NULL: THE PAIR RULE's rectangle */, int mask_cell,
                           const uint8_t* labels /* device, [n_rows][label_stride] */, int n_sims, int label_stride,
                           int64_t* sim_pairs /* [S][C][C][B] */, int32_t* sim_centres /* [S][C][B] */, int32_t* sim_inside /* [S][C] */,
                           int32_t* bd /* [M] */, int32_t* stats /* [2C+3], observed classes, as ay_pair_counts */,
                           void* workspace, size_t workspace_bytes, ay_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif
