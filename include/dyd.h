/*
 * dyd.h — C ABI of libdyd_gfx950.so, the MI355X (gfx950) device stage of the
 * annotation hot path of Cyclones-Y/Deal-Yolo-Daya.
 *
 * The reference (`src/deal_yolo_data/core/processor.py`) is pure Python and has no
 * FFI of its own; every entry point below replaces a Python loop or a pandas call of
 * that file and is what a ctypes binding added to the reference would bind
 * (INTEGRATION.md shows that binding).  Each declaration cites the reference lines
 * it replaces.
 *
 * Conventions
 *   - every function returns DYD_OK (0) or a negative DYD_ERR_* code; the message
 *     for the calling thread's last failure is dyd_last_error().  No C++ exception
 *     crosses this boundary.
 *   - all buffers are caller-owned and contiguous.  Functions without a suffix take
 *     HOST pointers and stage H2D / D2H themselves; `_dev` twins take DEVICE
 *     pointers (from dyd_malloc, or any hipMalloc'ed memory of the same device, e.g.
 *     a torch tensor's data_ptr) plus the hipStream_t to launch on, used as given
 *     (NULL = HIP's null stream).  `_dev` calls are asynchronous on that stream.
 *   - offsets arrays have n+1 entries, start at 0 and are non-decreasing.
 *   - the library keeps one lazily created context per process (device, stream,
 *     scratch); entry points are serialised by a process-wide mutex, so they may be
 *     called from any thread (Streamlit runs each session's script on its own
 *     thread: reference ui/pages/processing.py:200-213).
 */
#ifndef DYD_H
#define DYD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DYD_OK 0
#define DYD_ERR_INVALID (-1)   /* bad argument (null pointer, negative size, bad offsets) */
#define DYD_ERR_NO_DEVICE (-2) /* no gfx950 device visible / dyd_init failed */
#define DYD_ERR_HIP (-3)       /* a HIP runtime call or kernel launch failed */
#define DYD_ERR_OOM (-4)       /* device allocation failed */
#define DYD_ERR_RANGE (-5)     /* size exceeds what an int32 offset array can address */

/* keep modes of dyd_dedup == pandas drop_duplicates(keep=...) (processor.py:140-144) */
#define DYD_KEEP_FIRST 0
#define DYD_KEEP_LAST 1
#define DYD_KEEP_NONE 2

/* ---- context -------------------------------------------------------------------- */
int dyd_init(int device_or_minus1);
void dyd_shutdown(void);
const char *dyd_last_error(void);
int dyd_device_count(void);
const char *dyd_version(void);
/* name of the device the context is bound to ("" before dyd_init) */
const char *dyd_device_name(void);

/* ---- device memory + timing (for callers that keep data resident in HBM) -------- */
int dyd_malloc(void **dptr, size_t bytes);
int dyd_free(void *dptr);
int dyd_h2d(void *dst_dev, const void *src_host, size_t bytes);
int dyd_d2h(void *dst_host, const void *src_dev, size_t bytes);
int dyd_memset(void *dst_dev, int byte, size_t bytes);
int dyd_sync(void *stream);
/* Device-side failures (K4 / K5: hash table full, an inserted key not found again) are recorded in one status word on the device.
 * Host-pointer entry points check it themselves and return DYD_ERR_HIP; a caller of the asynchronous `_dev` twins asks here once its
 * launches are queued: synchronises `stream`, returns DYD_OK or DYD_ERR_HIP (message in dyd_last_error) and clears the word. */
int dyd_device_status(void *stream);
/* elapsed ms of the kernels launched by the calling thread's most recent non-_dev
 * entry point (hipEvent pair around the kernel launches only, staging excluded) */
double dyd_last_kernel_ms(void);

/* ---- K1: polygon ptList -> bbox -------------------------------------------------
 * Replaces get_bbox_points (processor.py:252-260), called per object at :273.
 * xy      : P points, interleaved (x,y) f64                       [2*P]
 * pt_off  : point offsets per box                                 [n_boxes+1]
 * out_box4: (min_x, min_y, max_x, max_y) per box                  [4*n_boxes]
 * out_arg4: index INSIDE the box of the point that supplies each of the four values,
 *           in the same order                                     [4*n_boxes]
 * Semantics are CPython's builtin min/max over the box's points in order: the FIRST
 * extremal element wins (strict < / > replaces the running best), so -0.0 vs 0.0 and
 * int-vs-float ties resolve to the lower index, and a NaN wins only from position 0.
 * A box with no points yields four NaNs and four -1 (the host emits JSON null,
 * processor.py:254-255). */
int dyd_bbox_minmax(const double *xy, const int32_t *pt_off, int64_t n_boxes,
                    double *out_box4, int32_t *out_arg4);
/* n_points = pt_off[n_boxes] (the table's shape picks the kernel: a lane per polygon for short polygons, sixteen lanes per
 * polygon from 48 points per polygon on); a negative value means "not known" and selects the short-polygon kernels. */
int dyd_bbox_minmax_dev(const double *xy, const int32_t *pt_off, int64_t n_boxes, int64_t n_points,
                        double *out_box4, int32_t *out_arg4, void *stream);

/* ---- K2: per-image box-count + all-pairs IoU filter ------------------------------
 * Replaces meet_conditions (processor.py:368-376) + calculate_iou (:328-339) and the
 * corner normalisation of extract_boxes (:359-362).
 * box4    : per box the two ptList points as stored (p1x, p1y, p2x, p2y); corners are
 *           re-normalised in the kernel with first-wins min/max       [4*B]
 * row_off : box offsets per image row                                  [n_rows+1]
 * out_high: 1 iff n_i >= min_boxes and some pair i<j has IoU >= thr    [n_rows]
 * out_max_iou_or_null: optional diagnostic, max pair IoU of the row (0.0 when the row
 *           has fewer than two boxes); not a reference output          [n_rows]
 * f64 arithmetic in the reference's operation order, no contraction, IEEE division. */
int dyd_iou_any_ge(const double *box4, const int32_t *row_off, int64_t n_rows,
                   int32_t min_boxes, double thr, uint8_t *out_high,
                   double *out_max_iou_or_null);
/* n_boxes = row_off[n_rows] (picks the kernel by the table's shape; negative: not known) */
int dyd_iou_any_ge_dev(const double *box4, const int32_t *row_off, int64_t n_rows, int64_t n_boxes,
                       int32_t min_boxes, double thr, uint8_t *out_high,
                       double *out_max_iou_or_null, void *stream);

/* ---- K9: greedy duplicate-box suppression inside each image row -------------------
 * For box j of a row: dropped iff some earlier box of the row that is itself kept has
 * calculate_iou(earlier, j) >= thr (processor.py:328-339 arithmetic, corners normalised as
 * in extract_boxes :359-362); with name_or_null only boxes of equal name id compare.
 * box4       : per box the two ptList points as stored (p1x, p1y, p2x, p2y)   [4*B]
 * row_off    : box offsets per image row                                     [n_rows+1]
 * name_or_null: optional name id per box (boxes compare iff the ids are equal)  [B]
 * out_keep   : 1 = kept, 0 = dropped                                         [B]
 * out_partner: in-row index of the first kept box that hit this one, or -1   [B] */
int dyd_suppress_boxes(const double *box4, const int32_t *row_off, int64_t n_rows,
                       const int32_t *name_or_null, double thr, uint8_t *out_keep,
                       int32_t *out_partner);
/* device pointers; n_boxes = row_off[n_rows] (required: it sizes the list of rows above 64 boxes) */
int dyd_suppress_boxes_dev(const double *box4, const int32_t *row_off, int64_t n_rows, int64_t n_boxes,
                           const int32_t *name_or_null, double thr, uint8_t *out_keep,
                           int32_t *out_partner, void *stream);

/* ---- K10: box audit — per-class box statistics of the YOLO step's boxes -------------
 * Per box (the labelled boxes of utils.py:681-710 with min/max corners, and the row's
 * width / height as processor.py:1013-1014 reads them): one category, tested in order
 *   0 no_size     the row's size_status is not 0 (1: `not w or not h`, :1023-1025; 2: not a
 *                 finite positive number)
 *   1 bad_coords  a corner is not finite (the caller encodes non-numbers as NaN)
 *   2 degenerate  bw = max(x2 - x1, 0.0) <= 0 or bh = max(y2 - y1, 0.0) <= 0 (:1052-1053)
 *   3 writable    everything else: out_of_image = x1 < 0 or y1 < 0 or x2 > W or y2 > H;
 *                 area bw * bh: small < 1024 <= medium < 9216 <= large; the line of :1056-1058
 *                 binned as bin(v) = min(max(floor(v * nbins), 0), nbins - 1) (in double) of
 *                 xc = (x1 + x2) / 2 / W, yc = (y1 + y2) / 2 / H, wn = bw / W, hn = bh / H.
 * Arithmetic in IEEE f64 without contraction.  A box whose class id is -1 (its name is no
 * str: it never equals a row label, :1006) gets only the unmatchable flag and row count.
 * box4       : per box (x1, y1, x2, y2) f64, 16-byte aligned                    [4*B]
 * row_off    : box offsets per image row                                       [n_rows+1]
 * cls        : class id per box, -1 or 0..n_classes-1 (_dev: others count as -1) [B]
 * width, height, size_status: per row f64, f64, u8 (0 ok, 1 missing, 2 invalid)  [n_rows]
 * n_classes >= 0, nbins in 1..64
 * out_flag   : bits 0-1 category, bit 2 out_of_image, bits 3-4 area bucket
 *              (0 small, 1 medium, 2 large; writable only), 0x80 = class id -1   [B]
 * out_row_counts: per row unmatchable, no_size, bad_coords, degenerate, writable,
 *              out_of_image                                                    [6*n_rows] i32
 * out_class_counts: per class no_size, bad_coords, degenerate, writable,
 *              out_of_image, small, medium, large, images (rows holding a box
 *              of the class)                                                   [9*n_classes] i64
 * out_hist_wh, out_hist_xy: [c][bin(wn)][bin(hn)], [c][bin(xc)][bin(yc)] over
 *              writable boxes                                      [n_classes*nbins*nbins] i64
 * out_boxes_per_image: rows with k boxes (all boxes), k = 256 takes >= 256       [257] i64 */
int dyd_box_audit(const double *box4, const int32_t *row_off, int64_t n_rows, const int32_t *cls,
                  const double *width, const double *height, const uint8_t *size_status,
                  int32_t n_classes, int32_t nbins, uint8_t *out_flag, int32_t *out_row_counts,
                  int64_t *out_class_counts, int64_t *out_hist_wh, int64_t *out_hist_xy,
                  int64_t *out_boxes_per_image);
/* device pointers; n_boxes = row_off[n_rows]; every output is written (the sums are zeroed first) */
int dyd_box_audit_dev(const double *box4, const int32_t *row_off, int64_t n_rows, int64_t n_boxes,
                      const int32_t *cls, const double *width, const double *height,
                      const uint8_t *size_status, int32_t n_classes, int32_t nbins, uint8_t *out_flag,
                      int32_t *out_row_counts, int64_t *out_class_counts, int64_t *out_hist_wh,
                      int64_t *out_hist_xy, int64_t *out_boxes_per_image, void *stream);

/* ---- K11: box repair — clip boxes to the image, drop the unusable ones ---------------
 * The box audit's boxes and inputs (K10).  Per box one action, the rules tested in order in
 * IEEE f64 without contraction:
 *   2 no_size         the row's size_status is not 0                      (box untouched)
 *   3 bad_coords      a corner is not finite                              (object removed)
 *   4 degenerate      max(x2 - x1, 0.0) <= 0 or max(y2 - y1, 0.0) <= 0     (object removed)
 *     then x1' = 0.0 if x1 < 0 else x1, y1' likewise, x2' = W if x2 > W else x2, y2' = H if
 *     y2 > H else y2, bw' = max(x2' - x1', 0.0), bh' likewise, clipped = x1 < 0 or y1 < 0 or
 *     x2 > W or y2 > H (K10's out_of_image)
 *   5 outside         bw' <= 0 or bh' <= 0                                (object removed)
 *   6 low_visibility  bw' * bh' < min_visibility * (bw * bh), bw = x2 - x1 (object removed)
 *   7 small           bw' < min_size or bh' < min_size                    (object removed)
 *   1 clip            clipped                                 (ptList -> (x1', y1'), (x2', y2'))
 *   0 keep            otherwise                                           (box untouched)
 * Geometry applies to every box; a box whose class id is -1 (its name is no str) is counted
 * per row only.
 * box4, row_off, cls, width, height, size_status: as dyd_box_audit
 * min_visibility in [0, 1], min_size finite and >= 0 (pixels)
 * out_action : bits 0-2 action code, 0x80 = class id -1                         [B] u8
 * out_box4   : per box the corners it is written with: (x1', y1', x2', y2') for
 *              code 1, the input corners otherwise; 16-byte aligned            [4*B] f64
 * out_row_counts: per row, per action code, over all boxes                   [8*n_rows] i32
 * out_class_counts: per class, per action code, over class ids >= 0         [8*n_classes] i64 */
int dyd_repair_boxes(const double *box4, const int32_t *row_off, int64_t n_rows, const int32_t *cls,
                     const double *width, const double *height, const uint8_t *size_status,
                     int32_t n_classes, double min_visibility, double min_size, uint8_t *out_action,
                     double *out_box4, int32_t *out_row_counts, int64_t *out_class_counts);
/* device pointers; n_boxes = row_off[n_rows]; every output is written (the sums are zeroed first) */
int dyd_repair_boxes_dev(const double *box4, const int32_t *row_off, int64_t n_rows, int64_t n_boxes,
                         const int32_t *cls, const double *width, const double *height,
                         const uint8_t *size_status, int32_t n_classes, double min_visibility,
                         double min_size, uint8_t *out_action, double *out_box4,
                         int32_t *out_row_counts, int64_t *out_class_counts, void *stream);

/* ---- K18: box comparison — match two box tables of the same image rows --------------
 * Tables A ("base") and B ("other") cover the same n_rows rows and share one class list.
 * iou(a, b) = calculate_iou(a, b) of processor.py:328-339 with the A box first (first-wins
 * max / min, intersection == 0 -> 0.0, IEEE f64 rounded operation by operation), corners
 * normalised as in extract_boxes :359-362.  Per row, independently, indices in-row:
 *   for j in 0 .. nb-1 (B boxes in annotation order: no scores exist, order ranks, as in K9):
 *     cand = { i : A box i not matched yet, (not by_label or a_cls[i] == b_cls[j]),
 *              iou(a_i, b_j) >= thr }
 *     cand not empty: i* = the i of cand with the largest iou, ties -> lowest i;
 *                     b_match[j] = i*, a_match[i*] = j, b_iou[j] = iou(a_i*, b_j)
 *     else:           b_match[j] = -1, b_iou[j] = 0.0
 *   a_match[i] = -1 for every A box never taken
 *   a_best[i] = max over ALL j of iou(a_i, b_j), b_best[j] = max over ALL i: class and
 *     matched state ignored; starts at 0.0 and is raised by `iou > best`, so a NaN IoU
 *     never raises it
 * A NaN IoU never matches (NaN >= thr is false); thr = NaN matches nothing; with thr <= 0 a
 * pair with empty intersection (IoU 0.0) is a candidate, as K2's and K9's.
 * a_box4, b_box4: per box the two points as stored (p1x, p1y, p2x, p2y), 16-byte aligned [4*B]
 * a_row_off, b_row_off: box offsets per image row                                 [n_rows+1]
 * a_cls, b_cls: class id per box, 0..n_classes-1 (_dev: a box with another id matches like
 *             any box but is left out of out_confusion)                               [B]
 * out_a_match [n_a] i32, out_b_match [n_b] i32, out_b_iou [n_b] f64, out_a_best [n_a] f64,
 * out_b_best [n_b] f64: as above
 * out_row_counts: per row matched with equal class, matched with different class, A
 *             unmatched, B unmatched                                        [4*n_rows] i32
 * out_confusion: (C+1) x (C+1) row-major, C = n_classes: a matched pair counts in
 *             [a_cls][b_cls], an unmatched A box in [a_cls][C], an unmatched B box in
 *             [C][b_cls]; [C][C] stays 0.  Zeroed by the entry.          [(C+1)*(C+1)] u64 */
int dyd_compare_boxes(const double *a_box4, const int32_t *a_row_off, const int32_t *a_cls,
                      const double *b_box4, const int32_t *b_row_off, const int32_t *b_cls,
                      int64_t n_rows, int32_t n_classes, double thr, int by_label,
                      int32_t *out_a_match, int32_t *out_b_match, double *out_b_iou,
                      double *out_a_best, double *out_b_best, int32_t *out_row_counts,
                      uint64_t *out_confusion);
/* device pointers; n_a = a_row_off[n_rows], n_b = b_row_off[n_rows] (required: they size the
 * list of rows that leave the tile kernel); n_rows == 0 returns at once, otherwise every
 * output is written (out_row_counts and out_confusion also when no row holds a box) */
int dyd_compare_boxes_dev(const double *a_box4, const int32_t *a_row_off, const int32_t *a_cls,
                          const double *b_box4, const int32_t *b_row_off, const int32_t *b_cls,
                          int64_t n_rows, int64_t n_a, int64_t n_b, int32_t n_classes, double thr,
                          int by_label, int32_t *out_a_match, int32_t *out_b_match,
                          double *out_b_iou, double *out_a_best, double *out_b_best,
                          int32_t *out_row_counts, uint64_t *out_confusion, void *stream);

/* ---- K24: scored box evaluation — COCO-style AP per class ----------------------------
 * After COCOeval's evaluateImg / accumulate for iouType "bbox", area range "all", no crowd
 * or ignore regions.  Table A holds the ground truth (GT), table B the detections, one
 * score each, over the same n_rows rows and one class list.  iou(g, d) is K18's (above),
 * the GT box first.  Host pointers only.
 * Selection, per row: a detection whose score is not finite is bad_score (state 2): it takes
 *   no part and is no false positive.  Scores compare as numbers, -0.0 equal to 0.0 (they
 *   are taken as score + 0.0 everywhere, also where an output reports one).  The others are
 *   ranked within (row, class) by score descending, ties to the earlier position in the row;
 *   rank >= max_dets is cut (state 1) and takes no part; the rest is evaluated (state 0).
 * Matching, per threshold index t on its own, lim = min(iou_thr[t], 1 - 1e-10): the row's
 *   evaluated detections in rank order (any interleaving of the classes: only equal classes
 *   match); detection d takes the GT box g of its row and class, still free at t, with the
 *   largest iou(g, d) >= lim, ties to the HIGHEST g (K18: the lowest).  A NaN IoU never
 *   matches; a GT box with a NaN corner still counts as ground truth.
 * gt_box4, dt_box4, *_row_off, *_cls: as K18's a_ / b_ tables        dt_score [n_dt] f64
 * iou_thr [T] f64, 1 <= T <= 32; max_dets >= 1
 * out_dt_state [n_dt] i32: 0 evaluated, 1 cut, 2 bad_score
 * out_dt_tp [n_dt] u32: bit t = matched at threshold t
 * out_dt_gt [n_dt] i32: in-row index of the GT box matched at t = 0, else -1
 * out_dt_iou [n_dt] f64: that pair's IoU, else 0.0
 * out_dt_best [n_dt] f64: largest IoU with any GT box of its row and class, free or not
 *             (from 0.0 by `iou > best`); 0.0 for a detection that is not evaluated
 * out_gt_hit [n_gt] u32: bit t = matched at threshold t
 * out_gt_best [n_gt] f64: largest IoU with any evaluated detection of its row and class
 * Every output element is written.  n_rows == 0 returns at once. */
int dyd_eval_match_boxes(const double *gt_box4, const int32_t *gt_row_off, const int32_t *gt_cls,
                         const double *dt_box4, const int32_t *dt_row_off, const int32_t *dt_cls,
                         const double *dt_score, int64_t n_rows, int32_t n_classes,
                         const double *iou_thr, int32_t T, int32_t max_dets,
                         int32_t *out_dt_state, uint32_t *out_dt_tp, int32_t *out_dt_gt,
                         double *out_dt_iou, double *out_dt_best, uint32_t *out_gt_hit,
                         double *out_gt_best);
/* Accumulation over the evaluated detections of a whole table in table order (n < 2^31,
 * finite scores): cls [n] i32, score [n] f64, tp [n] u32 (out_dt_tp), npig [C] i64 = GT boxes
 * per class, rec [R] f64 ascending recall points (R >= 1).  Per class c and threshold t:
 *   the detections of c by score descending, ties in table order; tp_k, fp_k = running counts
 *   after k+1 of them; rc_k = tp_k / npig; pr_k = tp_k / ((tp_k + fp_k) + 2^-52); pr replaced
 *   by its running maximum from the right; for each r the first k with rc_k >= rec[r]:
 *   precision[c,t,r] = pr_k, score_at[c,t,r] = score of k, both 0.0 without such a k;
 *   recall[c,t] = rc_last (0.0 without detections); ap[c,t] = (sum of precision[c,t,r] in
 *   ascending r) / R.  npig == 0: all of these are NaN.
 *   Operating point: over the k that end a run of equal scores, the largest
 *   f1_k = 2 tp_k / ((k+1) + npig), ties to the smallest k -> best_f1, best_score, best_tp,
 *   best_dets = k+1; NaN, NaN, 0, 0 when npig == 0 or c has no detection.
 * Integers and single correctly rounded f64 divisions in a fixed order: defined bit for bit.
 * out_precision, out_score_at [C*T*R] f64; out_recall, out_ap, out_best_f1, out_best_score
 * [C*T] f64; out_best_tp, out_best_dets [C*T] i64.  n_classes == 0 returns at once. */
int dyd_eval_accumulate(const int32_t *cls, const double *score, const uint32_t *tp, int64_t n,
                        int32_t n_classes, int32_t T, const int64_t *npig, const double *rec,
                        int32_t R, double *out_precision, double *out_score_at,
                        double *out_recall, double *out_ap, double *out_best_f1,
                        double *out_best_score, int64_t *out_best_tp, int64_t *out_best_dets);

/* ---- K1+K2 fused: poly -> bbox -> IoU flag in one pass ---------------------------
 * One launch that produces K1's outputs and K2's flag for rows whose boxes all come
 * from K1 (processing.py:580-598 runs the two steps back to back on the same rows).
 * box_off : box offsets per image row [n_rows+1], n_boxes = box_off[n_rows], n_points = pt_off[n_boxes]
 *           (or negative: not known); other arguments as K1 / K2.
 * The flag is the one the reference's two steps produce in sequence, not merely "K2 on K1's boxes": a polygon
 * without a valid point is written as a ptList of null coordinates by the replace step (processor.py:254-255), and
 * extract_boxes of the IoU step raises on it inside its blanket try (:359 -> :364-365), so the row's box list is the
 * PREFIX before that object — out_high[r] is computed over that prefix (out_box4 / out_arg4 still cover every box).
 * dyd_bbox_iou_fused is the host-pointer twin (stages the inputs, copies out_arg4 / out_high back, out_box4 only when
 * it is not NULL — the JSON emitter needs the arg indices, not the values). */
int dyd_bbox_iou_fused(const double *xy, const int32_t *pt_off, const int32_t *box_off, int64_t n_rows,
                       int32_t min_boxes, double thr, double *out_box4_or_null, int32_t *out_arg4,
                       uint8_t *out_high);
/* The same pass through a STAGING SLOT the caller holds across many calls: a stream, two timing events, a device arena and a
 * pinned host arena, all owned by the context and kept between calls (nothing is created, allocated or freed per pass once the
 * arenas have grown to the working size).  dyd_stage_acquire hands out a free slot — a new one while fewer than 64 exist, else it
 * waits — with its pinned arena grown to pinned_bytes if the budget (DYD_PINNED_POOL_MB, default 1024 for all slots together)
 * allows: *pinned / *pinned_cap tell what the caller got (possibly less, possibly nothing).  Host arrays of the _staged call may
 * lie inside that arena (then every copy is an asynchronous DMA) or anywhere else.  dyd_bbox_iou_fused is acquire(0) + staged +
 * release.  The native replace -> IoU pass (dyd_json_replace_iou) scans straight into the pinned arena. */
typedef struct dyd_stage dyd_stage;
int dyd_stage_acquire(size_t pinned_bytes, dyd_stage **out, void **pinned, size_t *pinned_cap);
void dyd_stage_release(dyd_stage *stage);
int dyd_bbox_iou_fused_staged(dyd_stage *stage, const double *xy, const int32_t *pt_off, const int32_t *box_off, int64_t n_rows,
                              int32_t min_boxes, double thr, double *out_box4_or_null, int32_t *out_arg4, uint8_t *out_high);
int dyd_bbox_iou_fused_dev(const double *xy, const int32_t *pt_off, const int32_t *box_off,
                           int64_t n_rows, int64_t n_boxes, int64_t n_points, int32_t min_boxes, double thr,
                           double *out_box4, int32_t *out_arg4, uint8_t *out_high, void *stream);

/* ---- K3: 128-bit hash of a string column -----------------------------------------
 * The equality test inside DataFrame.drop_duplicates (processor.py:140) and
 * Series.isin (:198) is replaced by equality of 128-bit hashes of the host's
 * canonical byte form of each cell (MurmurHash3 x64_128, seed 0).
 * bytes: concatenated cells; off: byte offsets [n+1]; out_hi_lo: (h1, h2) per row [2*n] */
int dyd_hash128(const uint8_t *bytes, const int64_t *off, int64_t n, uint64_t *out_hi_lo);
int dyd_hash128_dev(const uint8_t *bytes, const int64_t *off, int64_t n, uint64_t *out_hi_lo,
                    void *stream);

/* ---- K4: first / last / none-occurrence mask over hash keys ----------------------
 * Replaces drop_duplicates(subset=["source"], keep=keep) (processor.py:140-144).
 * h: (h1,h2) per row [2*n]; out_keep[i] = 1 iff row i survives. */
int dyd_dedup(const uint64_t *h, int64_t n, int keep_mode, uint8_t *out_keep);
int dyd_dedup_dev(const uint64_t *h, int64_t n, int keep_mode, uint8_t *out_keep, void *stream);

/* ---- K5: membership of main keys in a reference key set --------------------------
 * Replaces Series.isin(ref_values) (processor.py:194-199). out_mask[i] = 1 iff h[i] is
 * one of the r reference keys. */
int dyd_isin(const uint64_t *h, int64_t n, const uint64_t *ref_h, int64_t r, uint8_t *out_mask);
/* Verification of hash equality.  K4 / K5 call two cells equal when their 128-bit hashes are; pandas compares values
 * (processor.py:140-144, :198).  out_partner[i] = the first row whose hash equals row i's (i itself for a first occurrence) /
 * the reference row that main row i hit (-1: no hit); the host then compares the BYTES of every such pair
 * (dyd_host_cells_differ, multithreaded host code: cells given as flat text + offsets, optionally through index arrays; pairs with
 * a negative index are skipped; returns the number of pairs that differ, out_differs marks them) — zero means every match was a
 * match of values.  One extra gather per row on the device; the step functions do this by default (verify=True). */
int dyd_dedup_partner(const uint64_t *h, int64_t n, int64_t *out_partner);
int dyd_isin_partner(const uint64_t *h, int64_t n, const uint64_t *ref_h, int64_t r, int64_t *out_partner);
int64_t dyd_host_cells_differ(const uint8_t *text_a, const int64_t *off_a, const int64_t *idx_a, const uint8_t *text_b, const int64_t *off_b,
                              const int64_t *idx_b, int64_t n, int n_threads, uint8_t *out_differs_or_null);
int dyd_isin_dev(const uint64_t *h, int64_t n, const uint64_t *ref_h, int64_t r,
                 uint8_t *out_mask, void *stream);

/* ---- multi-GPU -------------------------------------------------------------------------------------------------
 * One process per GPU; rows are sharded contiguously; K1 / K2 / K7 need no communication.  The path's one real exchange — the
 * all-gather of each shard's locally unique 16-byte keys (and of the reference keys) — is issued by the host layer
 * (deal-yolo-daya_amd/distributed.py) through the process group the caller already has: torch.distributed with backend "nccl",
 * which IS RCCL over xGMI on ROCm, on the stream the `_dev` kernels run on.  SURVEY §8b sketched a library-owned communicator
 * (dyd_comm_init(nranks, rank, rccl_unique_id) + dyd_comm* variants); it is deliberately NOT part of this ABI: a second
 * bootstrap (unique-id exchange) and a second RCCL communicator beside the caller's, for a single all-gather, would duplicate
 * state the caller must own anyway (device binding, stream, process-group lifetime).  The library's side of a sharded call is
 * therefore the plain `_dev` entry points on the shard's arrays: dyd_hash128_dev, dyd_dedup_dev (shard-local pre-dedup),
 * dyd_isin_dev (probe of the local survivors against the other ranks' keys), dyd_split_ids_seeded_dev (with cat_rank_base),
 * and dyd_device_status.  dyd_dedup_global_dev below is the older form (every rank inserts ALL gathered keys). */

/* ---- multi-GPU dedup: keys of ALL ranks after the allgather ----------------------
 * all_h : gathered keys of every rank in global row order          [2*n_all]
 * first_global / n_local: this rank owns global rows [first_global, first_global+n_local)
 * out_keep: mask for the rank's own rows                             [n_local] */
int dyd_dedup_global_dev(const uint64_t *all_h, int64_t n_all, int64_t first_global,
                         int64_t n_local, int keep_mode, uint8_t *out_keep, void *stream);

/* ---- K6: train/val/test split ids -------------------------------------------------
 * Replaces DataFrame.sample(frac=1, random_state=seed) + the int(n*ratio) cuts per
 * category (processor.py:796-806).
 * dyd_mt19937_permutation is host code: numpy's legacy RandomState(seed).permutation(n)
 * (init_genrand + reversed Fisher-Yates with masked-rejection 32-bit draws).
 * cat            : category id per expanded row, -1 = unclassified     [n]
 * cat_perm_concat: per category its permutation, concatenated           [sum n_c]
 * cat_off        : start of each category inside cat_perm_concat        [n_cat+1]
 * n_train/n_val  : cut sizes per category                               [n_cat]
 * out_split      : 0 train / 1 val / 2 test / 255 unclassified          [n]
 * out_pos        : position of the row inside its shuffled category     [n] (-1 unclassified) */
int dyd_mt19937_permutation(uint32_t seed, int64_t n, int64_t *out);
int dyd_split_ids(const int32_t *cat, int64_t n, const int64_t *cat_perm_concat,
                  const int64_t *cat_off, const int64_t *n_train, const int64_t *n_val,
                  int32_t n_cat, uint8_t *out_split, int64_t *out_pos);
int dyd_split_ids_dev(const int32_t *cat, int64_t n, const int64_t *cat_perm_concat,
                      const int64_t *cat_off, const int64_t *n_train, const int64_t *n_val,
                      int32_t n_cat, uint8_t *out_split, int64_t *out_pos, void *stream);

/* ---- K8: the permutation itself on the device ------------------------------------------------------------------
 * numpy's legacy RandomState(seed).permutation(n) (what DataFrame.sample(frac=1, random_state=seed) shuffles with, :800) computed
 * in parallel on the GPU, identical to dyd_mt19937_permutation element for element: MT19937 stream by one workgroup, the masked
 * rejection resolved by iterated device-wide scans, the Fisher-Yates swap chain replaced by a closed form over one radix sort
 * (csrc/k8_perm.hip).  out_perm[k] = the value at shuffled position k, out_inverse[v] = the shuffled position of value v; either
 * may be NULL.  n <= 2^30.  Synchronous (it reads back a few words between rounds). */
int dyd_mt19937_permutation_dev(uint32_t seed, int64_t n, int64_t *out_perm_or_null, int64_t *out_inverse_or_null, void *stream);
/* K6 with the permutations made by K8 from `seed` (every category is shuffled with the same random_state, :800): no permutation
 * array crosses the boundary and no inversion pass is needed (K8 yields the inverse K6 looks positions up in).  cat_sizes /
 * n_train / n_val (and cat_rank_base for a shard, see dyd_split_ids_sharded_dev) are HOST arrays [n_cat]; cat / out_* as in
 * dyd_split_ids (device pointers for _dev, host pointers otherwise).  Synchronous. */
int dyd_split_ids_seeded(const int32_t *cat, int64_t n, uint32_t seed, const int64_t *cat_sizes, const int64_t *n_train,
                         const int64_t *n_val, int32_t n_cat, uint8_t *out_split, int64_t *out_pos);
int dyd_split_ids_seeded_dev(const int32_t *cat, int64_t n, uint32_t seed, const int64_t *cat_sizes_host, const int64_t *n_train_host,
                             const int64_t *n_val_host, int32_t n_cat, const int64_t *cat_rank_base_host_or_null, uint8_t *out_split,
                             int64_t *out_pos, void *stream);

/* multi-GPU K6: the rank holds a contiguous shard of the expanded rows; cat_rank_base[c] = number
 * of rows of category c held by lower ranks (from one allgather of per-rank category counts),
 * cat_off / perm / n_train / n_val describe the GLOBAL categories. */
int dyd_split_ids_sharded_dev(const int32_t *cat, int64_t n, const int64_t *cat_perm_concat,
                              const int64_t *cat_off, const int64_t *n_train, const int64_t *n_val,
                              int32_t n_cat, const int64_t *cat_rank_base, uint8_t *out_split,
                              int64_t *out_pos, void *stream);

/* ---- K7: YOLO label lines ----------------------------------------------
 * Replaces the per-box arithmetic and "%.6f" formatting of generate_yolo_datasets_from_excels
 * (processor.py:1046-1052) and the "\n".join of a row's lines (:1054):
 *   x1,x2 = min,max; y1,y2 = min,max; bw = max(x2-x1, 0.0); bh = max(y2-y1, 0.0); skip if bw<=0 or bh<=0;
 *   "{cid} {(x1+x2)/2/width:.6f} {(y1+y2)/2/height:.6f} {bw/width:.6f} {bh/height:.6f}"
 * box4         : boxes as (x1, y1, x2, y2) f64, any corner order              [4*n_boxes]
 * row_off      : boxes of row i are [row_off[i], row_off[i+1])               [n_rows+1]
 * sel_or_null  : 1 = the box carries the row's label (b[0] == label_value, :1006), NULL = all  [n_boxes]
 * width/height : the row's image size (:1013-1014)                            [n_rows]
 * class_id     : class_to_id[label_value] (:1049)                             [n_rows]
 * out_text_off : byte range of row i in the text = [off[i], off[i+1])         [n_rows+1]
 * out_flag     : 0 text written, 1 no line (the reference skips the row: 标注框无效 / 无匹配标签框),
 *                2 left to the host: zero width/height (the reference tests `not width` first, :1016),
 *                negative class id, or a value >= 2^43 whose "%.6f" has up to 316 characters  [n_rows]
 * dyd_yolo_lines     : host pointers; *out_text is allocated by the library (release with dyd_host_free).
 * dyd_yolo_lines_dev : device pointers; out_text_or_null == NULL only measures (offsets, flags, total);
 *                      otherwise text_cap bytes are available and DYD_ERR_RANGE is returned, with the needed
 *                      size in *out_total, when that is too little.  *out_total is a HOST int64.  n_boxes = row_off[n_rows]
 *                      (the table's shape picks the kernel; a negative value makes the entry read it back from the device). */
int dyd_yolo_lines(const double *box4, const int32_t *row_off, const uint8_t *sel_or_null,
                   const double *width, const double *height, const int32_t *class_id, int64_t n_rows,
                   int64_t *out_text_off, uint8_t *out_flag, uint8_t **out_text, int64_t *out_text_len);
int dyd_yolo_lines_dev(const double *box4, const int32_t *row_off, const uint8_t *sel_or_null,
                       const double *width, const double *height, const int32_t *class_id, int64_t n_rows,
                       int64_t n_boxes, int64_t *out_text_off, uint8_t *out_flag, uint8_t *out_text_or_null, int64_t text_cap,
                       int64_t *out_total, void *stream);

/* ---- K13: YOLO segmentation label lines --------------------------------------------------
 * One line per polygon that carries the row's label, "cls x1 y1 ... xn yn" (YOLO segment models), for
 * generate_yolo_datasets_from_excels(task="segment").  Per polygon, the first rule that applies gives its action:
 *   5 no_size        the row's width or height is not finite or not in (0, 2^43);
 *   2 bad_coords     a coordinate is not finite or |v| >= 2^43;
 *   3 too_few_points fewer than 2 points (two points become the four corners of their box);
 *   then Sutherland-Hodgman clips the points to [0, W] x [0, H] (passes x >= 0, x <= W, y >= 0, y <= H, each
 *   intersection from the edge's first point towards its second, IEEE f64 without contraction);
 *   4 empty          fewer than 3 clipped vertices, or a clipped width or height <= 0;
 *   1 clipped        some point lies outside the image;  0 written  otherwise;  255 the polygon is not selected.
 * A line is "{cls}" then " {n(x/W):.6f} {n(y/H):.6f}" per clipped vertex, n clamping to [0, 1] (8 bytes per value,
 * "%.6f" exact, ties to even), so digits(cls) + 18 * m bytes; a row's lines are joined with "\n".
 * xy           : points as given, (x, y) f64                                   [2*n_points]
 * pt_off       : points of polygon p are [pt_off[p], pt_off[p+1])             [n_polys+1]
 * row_off      : polygons of row i are [row_off[i], row_off[i+1])             [n_rows+1]
 * sel_or_null  : 1 = the polygon carries the row's label, NULL = all          [n_polys]
 * width/height : the row's image size                                         [n_rows]
 * class_id     : the row's class id                                           [n_rows]
 * out_text_off : byte range of row i in the text = [off[i], off[i+1])         [n_rows+1]
 * out_flag     : 0 text written, 1 no line, 2 left to the host (zero width / height, negative class id)  [n_rows]
 * out_action   : the codes above                                              [n_polys]
 * dyd_yolo_seg_lines     : host pointers; *out_text is allocated by the library (release with dyd_host_free).
 * dyd_yolo_seg_lines_dev : device pointers; out_text_or_null == NULL only measures (offsets, flags, actions, total);
 *                          otherwise text_cap bytes are available and DYD_ERR_RANGE is returned, with the needed size
 *                          in *out_total, when that is too little.  *out_total is a HOST int64.
 *                          n_polys = row_off[n_rows], n_points = pt_off[n_polys]. */
int dyd_yolo_seg_lines(const double *xy, const int32_t *pt_off, const int32_t *row_off, const uint8_t *sel_or_null,
                       const double *width, const double *height, const int32_t *class_id, int64_t n_rows,
                       int64_t *out_text_off, uint8_t *out_flag, uint8_t *out_action, uint8_t **out_text,
                       int64_t *out_text_len);
int dyd_yolo_seg_lines_dev(const double *xy, const int32_t *pt_off, const int32_t *row_off, const uint8_t *sel_or_null,
                           const double *width, const double *height, const int32_t *class_id, int64_t n_rows,
                           int64_t n_polys, int64_t n_points, int64_t *out_text_off, uint8_t *out_flag, uint8_t *out_action,
                           uint8_t *out_text_or_null, int64_t text_cap, int64_t *out_total, void *stream);

/* ---- K14: polygon audit — per-class polygon statistics and defects ---------------------------
 * Polygons: every object the YOLO step keeps (utils._extract_boxes_with_labels: named, non-empty ptList, the prefix kept on any
 * exception), whatever the row's label, with its points V = (float(x), float(y)) of every ptList dict holding both keys
 * (K13's rule; a value that is no number is NaN).  cls -1: the name is no str; the polygon is only counted as unmatchable
 * (category 255, defects 0, area NaN).  Per polygon:
 *   category     exactly K13's action (codes 0..5 of the K13 block, the same device code), with no_size for a row whose
 *                size_status is not 0 (missing or invalid, as _audit_sizes reads the size columns) or outside (0, 2^43);
 *   defects      written and clipped polygons only, bits:
 *                1 duplicate_vertices  len(V) >= 3 and some V[k] == V[k-1], cyclically, exact == (a closing point counts);
 *                2 self_intersecting   len(V) >= 3; U = V without cyclically consecutive duplicates, m = len(U) >= 3, and
 *                                      an adjacent edge pair doubles back (o(a,b,c) == 0 and (b-a).(c-b) < 0) or two
 *                                      non-adjacent edges share a point (a proper crossing by strict signs, or o == 0 with
 *                                      the point in the other segment's closed bounding box);
 *                                      o(p,q,r) = (q.x-p.x)*(r.y-p.y) - (q.y-p.y)*(r.x-p.x), on V as drawn;
 *                4 tiny_area           area < min_area;
 *   area         written and clipped: |s| * 0.5, s = sum_k (x_k*y_{k+1} - x_{k+1}*y_k) over K13's clipped vertices in their
 *                order (signed: the two loops of a bow-tie cancel); NaN otherwise.
 * All of it IEEE f64 without contraction.  The self-intersection test costs O(m^2) edge pairs per polygon (no sweep).
 * Per class c (u64): class_counts[c * 14 + j], j = 0 polygons, 1 images (rows holding a polygon of c), 2..7 one per
 * category code 0..5, 8..10 one per defect bit, 11..13 area small (< 32^2), medium (< 96^2), large over written and clipped;
 * hist_vertices[c * 11 + b] over len(V), upper bin edges 2, 3, 4, 8, 16, 32, 64, 128, 256, 1024, inf.
 * Inputs follow K13: xy [2*n_points] (16-B aligned), pt_off [n_polys+1], row_off [n_rows+1], cls [n_polys], width / height /
 * size_status [n_rows].  min_area finite and >= 0.
 * dyd_audit_polygons     : host pointers (n_polys = row_off[n_rows], n_points = pt_off[n_polys]);
 * dyd_audit_polygons_dev : device pointers, enqueued on stream (NULL: the library's stream). */
int dyd_audit_polygons(const double *xy, const int32_t *pt_off, const int32_t *row_off, const int32_t *cls, const double *width,
                       const double *height, const uint8_t *size_status, int64_t n_rows, int32_t n_classes, double min_area,
                       uint8_t *out_category, uint8_t *out_defects, double *out_area, int64_t *out_class_counts,
                       int64_t *out_hist_vertices);
int dyd_audit_polygons_dev(const double *xy, const int32_t *pt_off, const int32_t *row_off, const int32_t *cls, const double *width,
                           const double *height, const uint8_t *size_status, int64_t n_rows, int64_t n_polys, int64_t n_points,
                           int32_t n_classes, double min_area, uint8_t *out_category, uint8_t *out_defects, double *out_area,
                           int64_t *out_class_counts, int64_t *out_hist_vertices, void *stream);

/* ---- K16: COCO annotation objects from the annotation polygons (the COCO export step) --------
 * (K15 is not in use.)  Polygons are K14's, unchanged: every object the YOLO step keeps, V = (float(x), float(y)) of every
 * ptList dict holding both keys, a value that is no number NaN.  cat_id[p] >= 1 is the polygon's COCO category id;
 * cat_id[p] <= 0: the polygon is not selected (action 255).  width / height / size_status per row as K14 takes them.
 * Action, the first rule that applies:
 *   0..5  exactly K13's and K14's written, clipped, bad_coords, too_few_points, empty, no_size (no_size also for a row whose
 *         size_status is not 0): the same device code, two points become the four corners of their box, Sutherland-Hodgman
 *         clip to [0, W] x [0, H];
 *   6     too_large: a written or clipped polygon whose area is not < 2^43 (a polygon that winds round the image several
 *         times can exceed W * H; fix2 below is exact only below 2^43).
 * Only written and clipped polygons are printed.  area = K14's, |s| * 0.5 with the shoelace sum s over the clipped vertices C
 * in their order (bit for bit K14's area); out_area is NaN for a polygon that is not printed.
 * fix2(v), 0 <= v < 2^43, is the text of Python's "%.2f" % v: in IEEE f64 without contraction t = v * 100.0,
 * e = fma(v, 100.0, -t), n = (uint64)t, f = t - (double)n; n is rounded up when f > 0.5 or when f == 0.5 and (e > 0 or
 * (e == 0 and n is odd)); the text is n / 100, a dot and two digits of n % 100: max(digits(n), 3) + 1 bytes.
 * P = C with each coordinate clamped, px = 0.0 if not x > 0.0 else (W if x > W else x), py likewise with H (no -0.0, no
 * rounding overshoot of an intersection).  bx = min px, by = min py, bw = max px - bx, bh = max py - by.
 * Text of one polygon, no spaces:
 *   {"id":A,"image_id":I,"category_id":K,"bbox":[fix2(bx),fix2(by),fix2(bw),fix2(bh)],"area":fix2(area),"iscrowd":0,
 *    "segmentation":[[fix2(px0),fix2(py0),fix2(px1),...]]}
 * A = ann_id_base + the polygon's index in the call (over all polygons, selected or not: ids are unique and ascending, not
 * dense), I = image_id_base + the row's index, K = cat_id.  flags bit 0 clear: "segmentation":[] (the detect flavour; the box
 * is still the clipped polygon's).  The text of a call is the printed polygons in polygon order joined with "," (nothing
 * before the first or after the last; empty when none is printed).
 * Invalid arguments: a negative id base, image_id_base + n_rows >= 2^53, ann_id_base + n_polys >= 2^53.
 * xy [2*n_points] (16-B aligned), pt_off [n_polys+1], row_off [n_rows+1], cat_id [n_polys], width / height / size_status [n_rows].
 * out_action u8 [n_polys], out_area f64 [n_polys], out_row_kept i32 [n_rows] = the row's printed polygons.
 * dyd_coco_annotations     : host pointers; *out_text is allocated by the library (release with dyd_host_free).
 * dyd_coco_annotations_dev : device pointers; out_text_or_null == NULL only measures (actions, areas, row counts, total);
 *                            otherwise text_cap bytes are available and DYD_ERR_RANGE is returned, with the needed size in
 *                            *out_total, when that is too little.  *out_total is a HOST int64. */
#define DYD_COCO_SEGMENTATION 1u
int dyd_coco_annotations(const double *xy, const int32_t *pt_off, const int32_t *row_off, const int32_t *cat_id, const double *width,
                         const double *height, const uint8_t *size_status, int64_t n_rows, int64_t image_id_base, int64_t ann_id_base,
                         uint32_t flags, uint8_t *out_action, double *out_area, int32_t *out_row_kept, uint8_t **out_text,
                         int64_t *out_text_len);
int dyd_coco_annotations_dev(const double *xy, const int32_t *pt_off, const int32_t *row_off, const int32_t *cat_id,
                             const double *width, const double *height, const uint8_t *size_status, int64_t n_rows, int64_t n_polys,
                             int64_t n_points, int64_t image_id_base, int64_t ann_id_base, uint32_t flags, uint8_t *out_action,
                             double *out_area, int32_t *out_row_kept, uint8_t *out_text_or_null, int64_t text_cap, int64_t *out_total,
                             void *stream);

/* ---- K17: YOLO oriented-box label lines ---------------------------------------------------
 * One line per polygon that carries the row's label, "cls x1 y1 x2 y2 x3 y3 x4 y4" (YOLO OBB models), for
 * generate_yolo_obb_datasets_from_excels: the corners of a minimum-area rectangle that encloses the polygon.  Polygons,
 * points, sizes, sel and the class id are K13's, unchanged; actions 0..5 are exactly K13's (the same device code), 255 the
 * polygon is not selected; a two-point polygon is its box's four corners.  For a polygon K13 would write or clip, let
 * C = c_0..c_{m-1} be K13's clipped vertices in order.  All arithmetic is IEEE f64 without contraction in the order written;
 * every min or max replaces only on a strict comparison (the first value wins ties).
 *   1. start   s = the first vertex with the smallest y, among those the smallest x; cur = s.
 *   2. step    (gift wrapping, one pass over C) best = none; for each c_k in order whose coordinates differ from cur's:
 *              take it if best is none; else cr = (bx-cx)*(ky-cy) - (by-cy)*(kx-cx); take it when cr < 0, or when cr == 0 and
 *              (kx-cx)*(kx-cx) + (ky-cy)*(ky-cy) is strictly larger than best's.  No candidate: the walk ends.
 *   3. rectangle of the edge cur -> best, dx = bx-cx, dy = by-cy.  dx == 0 or dy == 0: the extent of C, corners
 *              (lx,ly),(hx,ly),(hx,hy),(lx,hy), area = (hx-lx)*(hy-ly).  Otherwise over all of C u = (x-cx)*dx + (y-cy)*dy,
 *              v = (y-cy)*dx - (x-cx)*dy, a = min u, b = max u, e = min v, f = max v, L = dx*dx + dy*dy,
 *              area = ((b-a)*(f-e))/L, and the corners for (u,v) in (a,e),(b,e),(b,f),(a,f) are
 *              (cx + (u*dx - v*dy)/L, cy + (u*dy + v*dx)/L).  The first rectangle is kept; a strictly smaller area replaces it.
 *   4. advance cur = best; the walk ends when cur has s's coordinates, or after m steps.
 *   6 flat     the kept area is not > 0 (collinear points): no line.  (K17's own code 6; K16's too_large is unrelated.)
 * clamped[p] = 1 when a kept corner has x < 0, x > W, y < 0 or y > H (the printer clamps it; Ultralytics rejects values
 * outside [0, 1]).  A line is "{cls}" then " {n(x/W):.6f} {n(y/H):.6f}" per corner, n and the printer K13's, so
 * digits(cls) + 72 bytes; a row's lines are joined with "\n".
 * xy (16-B aligned), pt_off, row_off, sel_or_null, width / height, class_id, out_text_off, out_flag: as K13.
 * out_action          : the codes above                                                  [n_polys]
 * out_clamped         : 1 = a corner of the polygon's line was clamped, else 0           [n_polys]
 * out_corners_or_null : x1 y1 .. x4 y4 in pixels, before clamping; untouched for a polygon without a line (16-B aligned
 *                       for the _dev entry)                                              [8*n_polys]
 * dyd_yolo_obb_lines     : host pointers; *out_text is allocated by the library (release with dyd_host_free).
 * dyd_yolo_obb_lines_dev : device pointers; out_text_or_null == NULL only measures (offsets, flags, actions, clamped,
 *                          corners, total); otherwise text_cap bytes are available and DYD_ERR_RANGE is returned, with the
 *                          needed size in *out_total, when that is too little.  *out_total is a HOST int64.
 *                          n_polys = row_off[n_rows], n_points = pt_off[n_polys]. */
int dyd_yolo_obb_lines(const double *xy, const int32_t *pt_off, const int32_t *row_off, const uint8_t *sel_or_null,
                       const double *width, const double *height, const int32_t *class_id, int64_t n_rows,
                       int64_t *out_text_off, uint8_t *out_flag, uint8_t *out_action, uint8_t *out_clamped,
                       double *out_corners_or_null, uint8_t **out_text, int64_t *out_text_len);
int dyd_yolo_obb_lines_dev(const double *xy, const int32_t *pt_off, const int32_t *row_off, const uint8_t *sel_or_null,
                           const double *width, const double *height, const int32_t *class_id, int64_t n_rows,
                           int64_t n_polys, int64_t n_points, int64_t *out_text_off, uint8_t *out_flag, uint8_t *out_action,
                           uint8_t *out_clamped, double *out_corners_or_null, uint8_t *out_text_or_null, int64_t text_cap,
                           int64_t *out_total, void *stream);

/* ---- K19: polygon simplification — Douglas-Peucker with segment distance (the polygon simplify step) ----
 * Polygons are K14's: every object the YOLO step keeps, V = (float(x), float(y)) of every ptList dict holding both keys, a
 * value that is no number NaN.  m = len(V), e2 = tolerance * tolerance.  All arithmetic is IEEE f64, operation by operation,
 * without contraction; the division is the correctly rounded one.  Only vertices are removed: no coordinate changes.
 * Action, the first that applies:
 *   2 bad_coords      a coordinate is not finite or |v| >= 2^43 (K13's bound): untouched;
 *   3 too_few_points  m < 4: untouched (a triangle cannot lose a point, two points are a box);
 *   otherwise the polygon is simplified as below: 1 simplified when some vertex is removed, else 0 kept.
 * Anchors: vertex 0, and b = the k maximising (x_k-x_0)*(x_k-x_0) + (y_k-y_0)*(y_k-y_0), ties to the lowest k.  When that
 * maximum is 0.0 (all points coincide) the polygon is kept, untouched.  The root segments are (0, b) and (b, m), index m
 * standing for vertex 0 (the closing chain).
 * Squared distance s(k; i, j), with P = V[i], Q = V[j mod m], dx = Q.x - P.x, dy = Q.y - P.y, ex = x_k - P.x, ey = y_k - P.y,
 * L2 = dx*dx + dy*dy:
 *   if L2 == 0.0, or t = dx*ex + dy*ey <= 0.0:  s = ex*ex + ey*ey
 *   else if t >= L2:                            fx = x_k - Q.x, fy = y_k - Q.y, s = fx*fx + fy*fy
 *   else                                        c = dx*ey - dy*ex, s = (c*c) / L2
 * For a segment with interior vertices (i < k < j), k* = the interior k with the largest s, ties to the lowest k, s* = that s.
 * The segment splits at k* when s* > e2: k* is kept and (i, k*), (k*, j) are treated the same way.  When neither root splits,
 * the root with the larger s* splits at its k* anyway (ties to (0, b); a root without interior vertices does not count): no
 * polygon drops below three vertices, and below that forced split the rule is plain Douglas-Peucker.  A split depends on its
 * segment alone, so every evaluation order (recursive, or in rounds over all current segments) gives the same bits.
 * Out: out_keep u8 [n_points] (1 = the vertex stays; all 1 for an untouched polygon), out_action u8 [n_polys], out_kept int32
 * [n_polys] (vertices that stay), out_dev2 f64 [n_polys] = the largest s* over the segments that ended without a split, 0.0
 * when nothing was removed: the largest squared distance of a removed vertex from the segment that replaced it, always <= e2.
 * Work: O(m * depth) distance evaluations per polygon, depth = the depth of the splits: O(m log m) for a round outline, O(m^2)
 * for a comb (like K14's pair test).  Polygons are tiered by m (a lane, a workgroup with the points in LDS, a workgroup
 * streaming from HBM; dyd_set_option "k19_lane_points", "k19_lds_points"); any m is exact.
 * xy [2*n_points] (16-B aligned), pt_off [n_polys+1].  tolerance finite, >= 0 and < 2^43, else DYD_ERR_INVALID.
 * dyd_simplify_polygons     : host pointers (n_points = pt_off[n_polys]);
 * dyd_simplify_polygons_dev : device pointers, enqueued on stream (NULL: the library's stream); every output is written. */
int dyd_simplify_polygons(const double *xy, const int32_t *pt_off, int64_t n_polys, double tolerance, uint8_t *out_keep,
                          uint8_t *out_action, int32_t *out_kept, double *out_dev2);
int dyd_simplify_polygons_dev(const double *xy, const int32_t *pt_off, int64_t n_polys, int64_t n_points, double tolerance,
                              uint8_t *out_keep, uint8_t *out_action, int32_t *out_kept, double *out_dev2, void *stream);

/* ---- K20: tiled YOLO label lines — every image row sliced into overlapping tiles (the tile step) ----
 * All arithmetic is IEEE f64, operation by operation, without contraction, as in K13.  The table is K16's: xy, pt_off, row_off,
 * width / height per row, and cls[p], the polygon's class id; cls[p] < 0: the polygon is not selected (action 255).
 * Parameters: integers tile_w, tile_h, step_x, step_y with 1 <= step <= tile <= 2^20; min_visibility finite and in [0, 1];
 * mode 0 segment, 1 detect; max_tiles_per_row in 1..2^20.  Anything else is DYD_ERR_INVALID.
 * Row status, the first rule that applies:
 *   1 no_size          K13's size test fails for W or H (not finite, not in (0, 2^43));
 *   2 fractional_size  W or H is not a whole number;
 *   3 too_many_tiles   nx * ny > max_tiles_per_row;
 *   0 tiled            otherwise.  Only rows of status 0 have tiles.
 * Grid, per axis, in int64, for a length L, tile T and step S: L <= T gives one tile, origin 0, extent L; otherwise
 * n = ceil((L - T) / S) + 1 tiles, tile j with origin min(j * S, L - T) and extent T (the last tile is moved back to end at the
 * image's edge: no tile leaves the image, nothing is padded).  A row's tiles are numbered ty * nx + tx; tile_off[i] is the
 * exclusive sum of the rows' tile counts, T = tile_off[n_rows] the number of tiles; T > 2^31 - 1 is DYD_ERR_RANGE.
 * Per polygon: action = exactly K13's on the row's W and H (codes 0..5, the same device code; 255 not selected).  Only written
 * and clipped polygons go on; A_img = K14's area of the image-clipped polygon.
 * Per tile (origin (ox, oy), extent (tw, th), taken as f64) and polygon, V = K13's vertex list (two points: the four corners):
 *   1. every vertex of V becomes (x - ox, y - oy);
 *   2. K13's clip, unchanged, with W = tw and H = th; 3. K13's walk over the clipped vertices C;
 *   4. `empty` (fewer than 3 vertices, or an extent of C that is not > 0): the polygon has no part in the tile;
 *   5. otherwise A_tile = the area of C (K14's);
 *   6. written in the tile when A_tile >= min_visibility * A_img (a product, so A_img == 0 always passes), 7. else dropped;
 *   8. a written polygon is cut when a moved vertex lies outside [0, tw] x [0, th].
 * So a tile's segment lines are exactly what K13 prints for the moved polygon in an image of tw x th.
 * Lines: segment "{cls}" then " {n(x/tw):.6f} {n(y/th):.6f}" per vertex of C (n and the printer K13's: digits(cls) + 18 * m
 * bytes); detect K7's line "{cls} {(x1+x2)/2/tw:.6f} {(y1+y2)/2/th:.6f} {(x2-x1)/tw:.6f} {(y2-y1)/th:.6f}" with (x1, y1, x2, y2)
 * the extent of C (every value lies in [0, 1 + 2^-50), DESIGN 5r has the argument, so it is 8 bytes, K13's printer prints it
 * as "%.6f" does, and the line is digits(cls) + 36 bytes).  A tile's lines are
 * its written polygons in polygon order joined with "\n"; the text is the tiles' texts one after the other, nothing between.
 * xy [2*n_points] (16-B aligned), pt_off [n_polys+1], row_off [n_rows+1], cls [n_polys], width / height [n_rows].
 * tiles_cap            : entries the caller provides in out_tile_line_count (out_text_off: one more).  T > tiles_cap is
 *                        DYD_ERR_RANGE with *out_n_tiles = T and out_row_status / out_tile_off written: size and call again
 *                        (or compute T from the rule above, as the origin and extent of tile g are computed).
 * out_row_status       : the codes above                                              u8  [n_rows]
 * out_tile_off         : tiles of row i are [off[i], off[i+1])                        i64 [n_rows+1]
 * out_tile_line_count  : lines of tile g                                              i32 [T]
 * out_text_off         : byte range of tile g in the text = [off[g], off[g+1])        i64 [T+1]
 * out_action           : K13's codes, 255                                             u8  [n_polys]
 * out_tiles_written / _cut / _dropped : tiles in which the polygon is written / written and cut / dropped   i32 [n_polys]
 * *out_n_tiles         : T (a HOST int64)
 * dyd_yolo_tile_lines     : host pointers; *out_text is allocated by the library (release with dyd_host_free).
 * dyd_yolo_tile_lines_dev : device pointers; out_text_or_null == NULL only measures (everything but the text);
 *                           otherwise text_cap bytes are available and DYD_ERR_RANGE is returned, with the needed size in
 *                           *out_total, when that is too little.  *out_total is a HOST int64.
 *                           n_polys = row_off[n_rows], n_points = pt_off[n_polys].
 * n_rows, n_polys, n_points and tiles_cap stay below 2^31 (DYD_ERR_INVALID otherwise). */
int dyd_yolo_tile_lines(const double *xy, const int32_t *pt_off, const int32_t *row_off, const int32_t *cls, const double *width,
                        const double *height, int64_t n_rows, int64_t tile_w, int64_t tile_h, int64_t step_x, int64_t step_y,
                        double min_visibility, int32_t mode, int64_t max_tiles_per_row, int64_t tiles_cap, uint8_t *out_row_status,
                        int64_t *out_tile_off, int32_t *out_tile_line_count, int64_t *out_text_off, uint8_t *out_action,
                        int32_t *out_tiles_written, int32_t *out_tiles_cut, int32_t *out_tiles_dropped, int64_t *out_n_tiles,
                        uint8_t **out_text, int64_t *out_text_len);
int dyd_yolo_tile_lines_dev(const double *xy, const int32_t *pt_off, const int32_t *row_off, const int32_t *cls, const double *width,
                            const double *height, int64_t n_rows, int64_t n_polys, int64_t n_points, int64_t tile_w, int64_t tile_h,
                            int64_t step_x, int64_t step_y, double min_visibility, int32_t mode, int64_t max_tiles_per_row,
                            int64_t tiles_cap, uint8_t *out_row_status, int64_t *out_tile_off, int32_t *out_tile_line_count,
                            int64_t *out_text_off, uint8_t *out_action, int32_t *out_tiles_written, int32_t *out_tiles_cut,
                            int32_t *out_tiles_dropped, int64_t *out_n_tiles, uint8_t *out_text_or_null, int64_t text_cap,
                            int64_t *out_total, void *stream);

/* ---- K21: label masks — the annotation polygons of every image row rasterised into one byte per pixel (the mask step) ----
 * All arithmetic is IEEE f64, operation by operation, without contraction, as in K13; the division is the correctly rounded one.
 * The table is K20's: xy, pt_off, row_off, width / height per row, and val[p] (int32), the byte painted for polygon p:
 * val[p] < 0: the polygon is not selected (action 255); val[p] > 255 is DYD_ERR_INVALID in the host entry and the caller's
 * duty in the _dev entry (the low byte is painted).
 * Parameters: background in 0..255; max_pixels_per_row in 1..2^30.  Anything else is DYD_ERR_INVALID.
 * Row status, the first rule that applies:
 *   1 no_size          K13's size test fails for W or H (not finite, not in (0, 2^43));
 *   2 fractional_size  W or H is not a whole number;
 *   3 too_large        W > max_pixels_per_row or H > max_pixels_per_row or W * H > max_pixels_per_row, tested in that order
 *                      (so nothing overflows);
 *   0 rasterised       otherwise.
 * pix_off[i] is the exclusive sum of W * H over the rows of status 0 (other rows add 0); total = pix_off[n_rows].  A row's mask
 * is H lines of W bytes at pix_off[i], row-major, no padding.
 * Polygon action, the first rule that applies:
 *   255 not selected    val[p] < 0;
 *   5 no_raster         the row's status is not 0;
 *   2 bad_coords        K13's rule: a coordinate is not finite or |v| >= 2^43;
 *   3 too_few_points    fewer than 2 points;
 *   0 rasterised        otherwise.  Only action 0 paints.
 * V is K13's vertex list (two points: the four corners (x1, y1), (x2, y1), (x2, y2), (x1, y2) of their box).
 * Coverage.  Pixel (i, j) has the centre xc = i + 0.5, yc = j + 0.5.  For each cyclic edge A = V[k], B = V[(k + 1) % m]:
 *   - canonical direction: if A.y > B.y, or A.y == B.y and A.x > B.x, the endpoints are swapped, giving P (the first) and Q;
 *   - an edge with P.y == Q.y never crosses; the edge crosses scanline j when P.y <= yc and yc < Q.y;
 *   - then t = yc - P.y, d = Q.x - P.x, n = t * d, q = n / (Q.y - P.y), xs = P.x + q.
 * The polygon covers the pixel when the number of crossing edges with xs > xc is odd (the even-odd rule; a centre on a left or
 * top edge is in, on a right or bottom edge out).  The canonical direction makes an edge shared by two polygons give the same
 * bits in both, so adjacent polygons neither overlap nor leave a gap.
 * Paint.  A pixel holds val[p] of the last polygon in table order (within its row) that covers it, background when none does.
 * Counters, i64 per polygon: covered[p] = the pixels of the image that p covers; owned[p] = the pixels that hold p's paint at the
 * end (ownership is by polygon: an equal val does not merge two polygons); both 0 unless the action is 0.
 * xy [2*n_points] (16-B aligned), pt_off [n_polys+1], row_off [n_rows+1], val [n_polys], width / height [n_rows].
 * out_row_status : the codes above                                  u8  [n_rows]
 * out_pix_off    : the mask of row i is bytes [off[i], off[i+1])    i64 [n_rows+1]
 * out_action     : the codes above                                  u8  [n_polys]
 * out_covered / out_owned                                           i64 [n_polys]
 * dyd_rasterize_polygons     : host pointers; *out_pixels is allocated by the library (release with dyd_host_free).
 * dyd_rasterize_polygons_dev : device pointers, enqueued on stream.  out_pixels_or_null == NULL only measures: status, pix_off,
 *                              action and *out_total (a HOST int64); the counters are not touched.  Otherwise pix_cap bytes are
 *                              available, and DYD_ERR_RANGE is returned, with the needed size in *out_total and no pixel or
 *                              counter written, when that is too little.  The pixel pointer may have any byte alignment.
 *                              n_polys = row_off[n_rows], n_points = pt_off[n_polys].
 * n_rows, n_polys and n_points stay below 2^31 (DYD_ERR_INVALID otherwise). */
int dyd_rasterize_polygons(const double *xy, const int32_t *pt_off, const int32_t *row_off, const int32_t *val, const double *width,
                           const double *height, int64_t n_rows, int32_t background, int64_t max_pixels_per_row,
                           uint8_t *out_row_status, int64_t *out_pix_off, uint8_t *out_action, int64_t *out_covered,
                           int64_t *out_owned, uint8_t **out_pixels, int64_t *out_pixels_len);
int dyd_rasterize_polygons_dev(const double *xy, const int32_t *pt_off, const int32_t *row_off, const int32_t *val, const double *width,
                               const double *height, int64_t n_rows, int64_t n_polys, int64_t n_points, int32_t background,
                               int64_t max_pixels_per_row, uint8_t *out_row_status, int64_t *out_pix_off, uint8_t *out_action,
                               int64_t *out_covered, int64_t *out_owned, uint8_t *out_pixels_or_null, int64_t pix_cap,
                               int64_t *out_total, void *stream);

/* ---- K22: polygon comparison — two polygon tables of the same image rows matched by mask IoU ----------------------------
 * Tables A ("base") and B ("other") are polygon tables in K21's layout: xy [2*P] f64 (16-B aligned), pt_off [B+1] i32, row_off
 * [n_rows+1] i32, and cls [B] i32: cls[p] < 0: the polygon is not selected, otherwise a class id in 0..n_classes-1 (a larger id is
 * DYD_ERR_INVALID in the host entry and the caller's duty in the _dev entry, where such a polygon takes part in everything but
 * the two matrices).  Both tables cover the same n_rows rows and share width / height [n_rows] f64.
 * Parameters: n_classes in 1..1023; max_pixels_per_row in 1..2^30; max_pairs_per_row in 1..2^24.  Anything else is
 * DYD_ERR_INVALID.  Offsets are clamped as K13 and K21 clamp them.
 * Row status, the first rule that applies:
 *   1 no_size, 2 fractional_size, 3 too_large   exactly K21's rules on W, H and max_pixels_per_row;
 *   4 too_many_pairs   na * nb > max_pairs_per_row, na and nb the row's polygon counts in A and B, selected or not;
 *   0 compared         otherwise.
 * Action per polygon, on either side, the first rule that applies (K21's codes): 255 not selected (cls < 0); 5 the row is not
 * compared; 2 bad_coords; 3 too_few_points; 0 compared.  Only polygons of action 0 take part in anything below.
 * Coverage.  cover(p) is K21's set of pixels: centre sampling, the canonical edge direction, P.y <= yc < Q.y,
 * xs = P.x + ((yc - P.y) * (Q.x - P.x)) / (Q.y - P.y) rounded operation by operation without contraction, the even-odd rule, a
 * two-point polygon taken as its box.
 * Pixel counts and IoU.  pixels[p] = |cover(p)|; inter(a, b) = |cover(a) & cover(b)|;
 *   iou(a, b) = (double)inter / (double)(pixels[a] + pixels[b] - inter) when inter > 0, else exactly 0.0.  There is no NaN IoU.
 * Matching, per row, indices in-row: K18's rule on that IoU with one difference: a pair is a candidate only when inter > 0 AND
 * iou >= thr, so a threshold <= 0 never matches disjoint polygons; thr = NaN matches nothing.
 *   for j in 0 .. nb-1 (compared B polygons in annotation order):
 *     cand = { i : A polygon i compared and not matched yet, (not by_label or a_cls[i] == b_cls[j]), inter(a_i, b_j) > 0,
 *              iou(a_i, b_j) >= thr }
 *     cand not empty: i* = the i of cand with the largest iou, ties -> lowest i; b_match[j] = i*, a_match[i*] = j, b_iou[j] = iou
 *     else:           b_match[j] = -1, b_iou[j] = 0.0
 *   a_match / b_match are -1 and b_iou 0.0 for every polygon never taken, compared or not.
 *   a_best[i] / b_best[j]: the largest iou with ANY compared polygon of the other side, class and matched state ignored; from 0.0.
 * out_confusion: K18's meaning over compared polygons: a matched pair in [a_cls][b_cls], an unmatched compared A polygon in
 *   [a_cls][C], an unmatched compared B polygon in [C][b_cls], C = n_classes.  out_row_counts: K18's four counts per row (matched
 *   with equal class, matched with different class, compared A unmatched, compared B unmatched).
 * Pixel classes.  On each side a pixel's class is the cls of the last compared polygon of the row, in table order, that covers it
 *   (K21's ownership), C (the background) when none does.  out_pixel_confusion[ca][cb] counts the pixels of all rows of status 0;
 *   its sum is the sum of W * H over those rows.  out_row_pixels: per row the pixels where both sides are foreground with the
 *   same class, then the pixels where either side is foreground.
 * Pair table.  pair_off[i] is the exclusive sum of na * nb over the rows of status 0 (other rows add 0).  inter(a_i, b_j) of row
 *   r is the u32 at pair_off[r] + i * nb + j (a row has at most 2^30 pixels).
 * out_row_status u8 [n_rows]; out_pair_off i64 [n_rows+1]; out_a_action / out_b_action u8 [B]; out_a_pixels / out_b_pixels i64
 * [B]; out_a_match / out_b_match i32 [B]; out_b_iou f64 [n_b]; out_a_best / out_b_best f64 [B]; out_row_counts i32 [4*n_rows];
 * out_confusion / out_pixel_confusion u64 [(C+1)*(C+1)], zeroed by the entry; out_row_pixels i64 [2*n_rows].
 * n_rows == 0 returns at once; otherwise every output is written, also when no row holds a polygon.
 * dyd_compare_polygons     : host pointers; the pair counts stay inside.
 * dyd_compare_polygons_dev : device pointers, enqueued on stream.  n_a = a_row_off[n_rows], n_a_points = a_pt_off[n_a], and the
 *                            same for B.  out_pairs_or_null: pair_cap u32 elements for the pair counts, left there for the
 *                            caller; NULL: the library keeps them in a buffer of its own.  DYD_ERR_RANGE when pair_off[n_rows]
 *                            exceeds pair_cap, DYD_ERR_OOM when the library's buffer cannot be had: in both cases nothing but
 *                            out_row_status and out_pair_off has been written.
 * n_rows, n_a, n_b and the point counts stay below 2^31 (DYD_ERR_INVALID otherwise). */
int dyd_compare_polygons(const double *a_xy, const int32_t *a_pt_off, const int32_t *a_row_off, const int32_t *a_cls,
                         const double *b_xy, const int32_t *b_pt_off, const int32_t *b_row_off, const int32_t *b_cls,
                         const double *width, const double *height, int64_t n_rows, int32_t n_classes, double thr, int by_label,
                         int64_t max_pixels_per_row, int64_t max_pairs_per_row, uint8_t *out_row_status, int64_t *out_pair_off,
                         uint8_t *out_a_action, uint8_t *out_b_action, int64_t *out_a_pixels, int64_t *out_b_pixels,
                         int32_t *out_a_match, int32_t *out_b_match, double *out_b_iou, double *out_a_best, double *out_b_best,
                         int32_t *out_row_counts, uint64_t *out_confusion, uint64_t *out_pixel_confusion, int64_t *out_row_pixels);
int dyd_compare_polygons_dev(const double *a_xy, const int32_t *a_pt_off, const int32_t *a_row_off, const int32_t *a_cls,
                             const double *b_xy, const int32_t *b_pt_off, const int32_t *b_row_off, const int32_t *b_cls,
                             const double *width, const double *height, int64_t n_rows, int64_t n_a, int64_t n_a_points, int64_t n_b,
                             int64_t n_b_points, int32_t n_classes, double thr, int by_label, int64_t max_pixels_per_row,
                             int64_t max_pairs_per_row, uint8_t *out_row_status, int64_t *out_pair_off, uint8_t *out_a_action,
                             uint8_t *out_b_action, int64_t *out_a_pixels, int64_t *out_b_pixels, int32_t *out_a_match,
                             int32_t *out_b_match, double *out_b_iou, double *out_a_best, double *out_b_best,
                             int32_t *out_row_counts, uint64_t *out_confusion, uint64_t *out_pixel_confusion, int64_t *out_row_pixels,
                             uint32_t *out_pairs_or_null, int64_t pair_cap, void *stream);

/* ---- K25: scored polygon evaluation — COCO-style mask AP per class: K24's selection and matching on K22's mask IoU ---------
 * After COCOeval's evaluateImg for iouType "segm", area range "all", no crowd or ignore regions.  Table A holds the ground truth
 * (GT), table B the detections, both polygon tables in K22's layout (xy, pt_off, row_off, cls with cls < 0 = not selected) over
 * the same n_rows rows, width / height [n_rows] f64 and one class list; dt_score [n_dt] f64 holds one score per detection.
 * Host pointers only; the pair table stays inside the library.  The accumulation is dyd_eval_accumulate (K24), unchanged.
 * Parameters: 1 <= T <= 32; max_dets >= 1; n_classes in 1..1023; max_pixels_per_row in 1..2^30; max_pairs_per_row in 1..2^24; a
 * class id >= n_classes: anything else is DYD_ERR_INVALID.
 * Rows and polygons.  Row status (status 4 too_many_pairs included), the action per polygon, cover(p), pixels[p] and
 *   inter(g, d) are exactly K22's.  iou(g, d) = (double)inter / (double)(pixels[g] + pixels[d] - inter) when inter > 0, else
 *   exactly 0.0: one correctly rounded division, no NaN IoU.  Only polygons of action 0 (in rows of status 0) take part.
 * Detection state: 3 skipped: the action is not 0 (not selected, row not evaluated, bad_coords, too_few_points).  2 bad_score:
 *   the score is not finite.  The others are ranked within (row, class) by score descending, ties to the earlier position in the
 *   row, -0.0 equal to 0.0 (score + 0.0 everywhere, also where an output reports a score): 1 cut: rank >= max_dets;
 *   0 evaluated: the rest.
 * Matching, per threshold index t on its own, lim = min(iou_thr[t], 1 - 1e-10): the row's evaluated detections in score order
 *   (any interleaving of the classes); detection d takes the GT polygon g of its row and class (action 0) that is still free
 *   at t, has inter(g, d) > 0 and the largest iou(g, d) >= lim, ties to the HIGHEST g (K24's rule; K22 takes the lowest).  A
 *   NaN threshold matches nothing.
 * Ground truth.  A GT polygon of action 0 counts as ground truth also when it covers no pixel centre; it can never be matched.
 *   A GT polygon of any other action is no ground truth (the caller reports it as skipped).  A detection that covers no pixel
 *   is evaluated and is a false positive at every threshold.
 * out_row_status u8 [n_rows], out_pair_off i64 [n_rows+1], out_gt_action / out_dt_action u8, out_gt_pixels / out_dt_pixels i64:
 *   K22's out_row_status, out_pair_off, out_a_action / out_b_action and out_a_pixels / out_b_pixels
 * out_dt_state [n_dt] i32: the codes above
 * out_dt_tp [n_dt] u32: bit t = matched at threshold t
 * out_dt_gt [n_dt] i32: in-row index of the GT polygon matched at t = 0, else -1
 * out_dt_iou [n_dt] f64: that pair's IoU, else 0.0
 * out_dt_best [n_dt] f64: largest IoU with any GT polygon of its row and class of action 0, free or not; 0.0 for a detection
 *             that is not evaluated
 * out_gt_hit [n_gt] u32: bit t = matched at threshold t
 * out_gt_best [n_gt] f64: largest IoU over the evaluated detections of its row and class
 * Every output element is written, also in rows that are not evaluated (0, -1 and 0.0).  n_rows == 0 returns at once. */
int dyd_eval_match_polygons(const double *gt_xy, const int32_t *gt_pt_off, const int32_t *gt_row_off, const int32_t *gt_cls,
                            const double *dt_xy, const int32_t *dt_pt_off, const int32_t *dt_row_off, const int32_t *dt_cls,
                            const double *dt_score, const double *width, const double *height, int64_t n_rows, int32_t n_classes,
                            const double *iou_thr, int32_t T, int32_t max_dets, int64_t max_pixels_per_row,
                            int64_t max_pairs_per_row, uint8_t *out_row_status, int64_t *out_pair_off, uint8_t *out_gt_action,
                            uint8_t *out_dt_action, int64_t *out_gt_pixels, int64_t *out_dt_pixels, int32_t *out_dt_state,
                            uint32_t *out_dt_tp, int32_t *out_dt_gt, double *out_dt_iou, double *out_dt_best, uint32_t *out_gt_hit,
                            double *out_gt_best);

/* ---- K23: COCO RLE — the column-major run lengths of every selected polygon's own mask, as COCO's "counts" string --------
 * The table is K21's: xy [2*P] f64 (16-B aligned), pt_off [B+1] i32, row_off [n_rows+1] i32, width / height [n_rows] f64, and
 * sel [B] i32: sel[p] < 0: the polygon is not selected (action 255); any other value selects it.  max_pixels_per_row in 1..2^30,
 * anything else is DYD_ERR_INVALID.  Offsets are clamped as K13 and K21 clamp them.
 * Row status: K21's, unchanged (0 encoded, 1 no_size, 2 fractional_size, 3 too_large).
 * Polygon action: K21's, unchanged (255 not selected, 5 no_raster, 2 bad_coords, 3 too_few_points, 0 encoded).
 * Coverage.  cover(p, i, j) is K21's, bit for bit, of polygon p alone: no polygon hides another.
 * Runs.  For a polygon of action 0 in an image of W x H, pixel (i, j) has the column-major index k = i * H + j.  Let
 * t_0 < t_1 < ... < t_{m-1} be the indices k in [0, W*H) at which cover(k) != cover(k - 1), taking cover(-1) = 0.  The runs are
 * t_0, t_1 - t_0, ..., W*H - t_{m-1}: m + 1 values, alternating zeros and ones, starting with zeros (the first run is 0 when pixel
 * (0, 0) is covered; a polygon that covers nothing has the single run W*H; a run continues from the bottom of one column into
 * the top of the next).  Runs are u32, every value at most 2^30.  A polygon whose action is not 0 has no runs.
 * String.  COCO's rleToString over the runs c_0 .. c_m: for run i take x = c_i, or x = c_i - c_{i-2} when i > 2 (x is signed);
 * repeat { b = x & 0x1f; x >>= 5 (arithmetic); more = (b & 0x10) ? x != -1 : x != 0; if (more) b |= 0x20; emit the byte b + 48 }
 * while more.  At most 7 bytes per run.  {"size": [H, W], "counts": <the string>} is the polygon's COCO "segmentation".
 * Area and box.  area[p] is the number of covered pixels (K21's covered[p]); bbox[4p ..] = x, y, w, h of the covered pixels (min
 * column, min line, extent), all 0 when the area is 0.  Both are 0 unless the action is 0.
 * out_row_status : the codes above                                        u8  [n_rows]
 * out_action     : the codes above                                        u8  [n_polys]
 * out_area                                                                i64 [n_polys]
 * out_bbox                                                                i32 [4*n_polys]
 * out_run_off    : the runs of polygon p are runs[off[p] .. off[p+1])     i64 [n_polys+1]
 * runs                                                                    u32 [run_off[n_polys]]
 * out_text_off   : the string of polygon p is text[off[p] .. off[p+1])    i64 [n_polys+1]
 * text                                                                    u8  [text_off[n_polys]]
 * dyd_polygon_rle     : host pointers; *out_runs (*out_runs_len values) and *out_text are allocated by the library (release each
 *                       with dyd_host_free).
 * dyd_polygon_rle_dev : device pointers.  It takes NO stream: it hands totals to the host, so it is blocking in any case; it
 *                       runs on the library's own stream and waits for it before it returns.  A caller whose inputs were produced
 *                       on another stream synchronises that stream first.
 *                       out_runs_or_null == NULL only measures the runs: status, action, area, bbox, run_off and *out_run_total
 *                       (a HOST int64); out_text_off may then be NULL.  With runs but out_text_or_null == NULL it also fills the
 *                       runs, text_off and *out_text_total (a HOST int64).  With both it produces everything.  When runs_cap
 *                       (values) or text_cap (bytes) is too small, DYD_ERR_RANGE is returned with the needed size in the total
 *                       and nothing of that output written.  Output pointers may have any alignment their type allows.
 *                       n_polys = row_off[n_rows], n_points = pt_off[n_polys].
 * n_rows, n_polys and n_points stay below 2^31 (DYD_ERR_INVALID otherwise). */
int dyd_polygon_rle(const double *xy, const int32_t *pt_off, const int32_t *row_off, const int32_t *sel, const double *width,
                    const double *height, int64_t n_rows, int64_t max_pixels_per_row, uint8_t *out_row_status, uint8_t *out_action,
                    int64_t *out_area, int32_t *out_bbox, int64_t *out_run_off, int64_t *out_text_off, uint32_t **out_runs,
                    int64_t *out_runs_len, uint8_t **out_text, int64_t *out_text_len);
int dyd_polygon_rle_dev(const double *xy, const int32_t *pt_off, const int32_t *row_off, const int32_t *sel, const double *width,
                        const double *height, int64_t n_rows, int64_t n_polys, int64_t n_points, int64_t max_pixels_per_row,
                        uint8_t *out_row_status, uint8_t *out_action, int64_t *out_area, int32_t *out_bbox, int64_t *out_run_off,
                        uint32_t *out_runs_or_null, int64_t runs_cap, int64_t *out_text_off, uint8_t *out_text_or_null,
                        int64_t text_cap, int64_t *out_run_total, int64_t *out_text_total);

/* ---- native flatten / emit (HOST code, multithreaded) ------------------------------
 * Schema-specialised JSON scanner + canonical re-emitter that replaces json.loads / json.dumps inside
 * parse_and_replace_ptlist (processor.py:262-281), extract_width_height (:285-292) and extract_boxes
 * (:341-366).  Cells are passed as concatenated UTF-8 text + offsets; `missing[i]` marks NaN cells.
 * status per cell: 0 regular, 1 undecodable JSON (the reference yields None / no boxes), 2 irregular
 * (the caller must process the cell with the Python flatten of flatten.py), 3 missing.
 * The handle owns every array the accessors return; free it with dyd_scan_free. */
typedef struct dyd_scan dyd_scan;
int dyd_json_scan_polygons(const uint8_t *text, const int64_t *cell_off, const uint8_t *missing,
                           int64_t n_cells, int n_threads, dyd_scan **out);
int dyd_json_emit_polygons(dyd_scan *scan, const uint8_t *text, const int64_t *cell_off,
                           const int32_t *arg4, int n_threads, const uint8_t **out_text,
                           const int64_t **out_off);
int dyd_json_scan_boxes(const uint8_t *text, const int64_t *cell_off, const uint8_t *missing,
                        int64_t n_cells, int n_threads, dyd_scan **out);
/* Duplicate-box suppression: dyd_json_scan_boxes' walk (same boxes, prefix-on-exception rule and status) plus, per box,
 * dyd_scan_box_object = index of its object in "objects" and dyd_scan_box_name = a name id local to the cell (equal ids <=>
 * equal decoded names; -1 = no "name" or null).  A box whose "name" is neither a string nor null makes the cell irregular.
 * The _v form takes one (pointer, length) per cell; the pointers must stay valid until dyd_scan_free. */
int dyd_json_scan_box_objects(const uint8_t *text, const int64_t *cell_off, const uint8_t *missing,
                              int64_t n_cells, int n_threads, dyd_scan **out);
int dyd_json_scan_box_objects_v(const uint8_t *const *cell_ptr, const int64_t *cell_len, const uint8_t *missing,
                                int64_t n_cells, int n_threads, dyd_scan **out);
const int32_t *dyd_scan_box_object(const dyd_scan *scan);   /* [n_boxes] */
const int32_t *dyd_scan_box_name(const dyd_scan *scan);     /* [n_boxes] */
/* After dyd_json_scan_box_objects: for every cell with at least one drop_per_box[b] set, the whole document as
 * json.dumps(..., ensure_ascii=False) writes it with those boxes' objects left out.  out_changed[i] (caller's, [n_cells]):
 * 0 unchanged (empty text), 1 text written, 2 the cell could not be re-spelled natively (the caller decides it).  The text
 * and its offsets [n_cells+1] are owned by the handle. */
int dyd_json_emit_dropping(dyd_scan *scan, const uint8_t *drop_per_box, int n_threads, uint8_t *out_changed,
                           const uint8_t **out_text, const int64_t **out_off);
int64_t dyd_scan_n_boxes(const dyd_scan *scan);
int64_t dyd_scan_n_points(const dyd_scan *scan);
const double *dyd_scan_xy(const dyd_scan *scan);              /* points [2*P] (polygons) or box4 [4*B] (boxes) */
const int32_t *dyd_scan_pt_off(const dyd_scan *scan);         /* [n_boxes+1] */
const int32_t *dyd_scan_cell_box_off(const dyd_scan *scan);   /* [n_cells+1] */
const uint8_t *dyd_scan_status(const dyd_scan *scan);         /* [n_cells] */
const uint8_t *dyd_scan_wh_kind(const dyd_scan *scan, int which);   /* which: 0 width, 1 height; 0 none 1 int 2 float 3 other */
const double *dyd_scan_wh_value(const dyd_scan *scan, int which);
/* polygon scan only, [n_cells]: 1 = some coordinate of the cell is an int beyond 2^25.  calculate_iou (processor.py:328-339)
 * multiplies coordinate differences in CPython's exact int arithmetic; f64 follows it only while every product stays below
 * 2^53, so the fused K1+K2 flag of such a cell is not used: the host decides it from the emitted boxes (flatten.py). */
const uint8_t *dyd_scan_iou_host(const dyd_scan *scan);
/* polygon scan only: how many cells the single-parse lane (csrc/host_json_fast.h) took; the others went through the exact walker */
int64_t dyd_scan_fast_cells(const dyd_scan *scan);
/* dyd_json_scan_polygons over one (pointer, length) pair per cell instead of a flat buffer — e.g. the UTF-8 views of a DataFrame
 * column's str objects, so that no cell is copied.  The pointers must stay valid until dyd_scan_free; dyd_json_emit_polygons may
 * then be called with text == cell_off == NULL. */
int dyd_json_scan_polygons_v(const uint8_t *const *cell_ptr, const int64_t *cell_len, const uint8_t *missing, int64_t n_cells,
                             int n_threads, dyd_scan **out);
/* YOLO step (utils.py:681-710, processor.py:1006): per cell the (min x, min y, max x, max y) of every named object
 * with a non-empty ptList, in dyd_scan_xy as box4, and dyd_scan_sel[b] = 1 when the object's name equals the row's
 * label value (label_text / label_off: one label per cell).  Undecodable cells give no boxes, like the reference's
 * blanket except; status 2 cells are left to the Python path. */
int dyd_json_scan_labelled(const uint8_t *text, const int64_t *cell_off, const uint8_t *missing, int64_t n_cells,
                           const uint8_t *label_text, const int64_t *label_off, int n_threads, dyd_scan **out);
const uint8_t *dyd_scan_sel(const dyd_scan *scan);             /* [n_boxes] (labelled scan only) */
/* Segmentation labels: the labelled scan's walk (same objects, irregular cells and statuses) that also keeps each
 * object's polygon: dyd_scan_xy = its points (x, y) as f64 [2*n_points], every ptList entry that is a dict holding both
 * "x" and "y", in order; dyd_scan_pt_off [n_boxes+1]; dyd_scan_sel and dyd_scan_cell_box_off as dyd_json_scan_labelled.
 * The _v form takes one (pointer, length) per cell. */
int dyd_json_scan_labelled_polygons(const uint8_t *text, const int64_t *cell_off, const uint8_t *missing, int64_t n_cells,
                                    const uint8_t *label_text, const int64_t *label_off, int n_threads, dyd_scan **out);
int dyd_json_scan_labelled_polygons_v(const uint8_t *const *cell_ptr, const int64_t *cell_len, const uint8_t *missing,
                                      int64_t n_cells, const uint8_t *label_text, const int64_t *label_off, int n_threads,
                                      dyd_scan **out);
/* Box audit: the labelled scan's walk (same boxes, same irregular cells) without a row label; per box
 * dyd_scan_box_object = index of its object in "objects" and dyd_scan_box_name = a table-wide class id, numbered
 * by first occurrence in cell order whatever the thread count.  The decoded names (UTF-8) of the ids are
 * dyd_scan_names: n_names, then bytes and offsets [n_names+1] owned by the handle.  Numbers, true and containers
 * as "name" make the cell irregular; the _v form takes one (pointer, length) per cell. */
int dyd_json_scan_named_boxes(const uint8_t *text, const int64_t *cell_off, const uint8_t *missing,
                              int64_t n_cells, int n_threads, dyd_scan **out);
int dyd_json_scan_named_boxes_v(const uint8_t *const *cell_ptr, const int64_t *cell_len, const uint8_t *missing,
                                int64_t n_cells, int n_threads, dyd_scan **out);
int64_t dyd_scan_names(const dyd_scan *scan, const uint8_t **text, const int64_t **off);
/* Polygon audit (K14): the named-box scan's objects, names and class ids with the points of each (the labelled-polygon
 * scan's dyd_scan_xy = (x, y) per point and dyd_scan_pt_off), see K14 above; same irregular cells. */
int dyd_json_scan_named_polygons(const uint8_t *text, const int64_t *cell_off, const uint8_t *missing,
                                 int64_t n_cells, int n_threads, dyd_scan **out);
int dyd_json_scan_named_polygons_v(const uint8_t *const *cell_ptr, const int64_t *cell_len, const uint8_t *missing,
                                   int64_t n_cells, int n_threads, dyd_scan **out);
/* Box repair, after dyd_json_scan_named_boxes(_v): for every cell with a box whose action (bits 0-2 of
 * action_per_box, K11's codes) is 1 or 3..7, the whole document as json.dumps(..., ensure_ascii=False) writes it
 * with the objects of codes 3..7 left out and, for code 1, the object's polygon.ptList replaced by
 * [{"x": x1', "y": y1'}, {"x": x2', "y": y2'}] from box4 [4*n_boxes] (float repr).  out_changed, text and
 * offsets as dyd_json_emit_dropping. */
int dyd_json_emit_repaired(dyd_scan *scan, const uint8_t *action_per_box, const double *box4, int n_threads,
                           uint8_t *out_changed, const uint8_t **out_text, const int64_t **out_off);
/* Polygon simplification, after dyd_json_scan_named_polygons(_v): keep_per_point [n_points] is K19's out_keep over the scan's
 * points.  For every cell holding a polygon with a vertex that is not kept, the whole document as json.dumps(...,
 * ensure_ascii=False) writes it, with each such object's polygon.ptList lacking the entries of those vertices; ptList entries
 * that are no vertices (non-dicts, dicts lacking "x" or "y") stay in place.  out_changed, text and offsets as
 * dyd_json_emit_dropping (2: the caller re-spells the cell, flatten.simplify_cell). */
int dyd_json_emit_simplified(dyd_scan *scan, const uint8_t *keep_per_point, int n_threads, uint8_t *out_changed,
                             const uint8_t **out_text, const int64_t **out_off);
/* The replace step and the IoU step in ONE native pass (processor.py:262-281 then :341-376; ui/pages/processing.py:580-598 runs them
 * back to back): cells as flat text + offsets, or as one (pointer, length) pair per cell (text == cell_off == NULL).  Every worker
 * thread holds one staging slot (dyd_stage_acquire) and takes its share of the cells through scan -> dyd_bbox_iou_fused_staged -> emit
 * chunk by chunk (DYD_PIPE_CHUNK_KB of cell text, default 8192), the points scanned straight into the slot's pinned arena.  The handle then
 * holds per cell: dyd_scan_status, dyd_scan_high (the IoU step's flag, meaningful for status 0 cells; the caller decides cells with
 * dyd_scan_iou_host != 0 and status 2 cells itself), dyd_scan_wh_*; and the emitted text per part (dyd_scan_part) or gathered
 * (dyd_scan_text).  Needs the device (no CPU fallback). */
int dyd_json_replace_iou(const uint8_t *text, const int64_t *cell_off, const uint8_t *const *cell_ptr, const int64_t *cell_len,
                         const uint8_t *missing, int64_t n_cells, int32_t min_boxes, double thr, int n_threads, dyd_scan **out);
/* Emitted text outlives the pass that wrote it; a freed handle parks those blocks (up to DYD_HOST_POOL_MB, default 3072) so that the
 * next pass writes into warm memory instead of tearing 2 GB of page tables down and faulting them in again.  This gives them back. */
void dyd_host_pool_trim(void);
const uint8_t *dyd_scan_high(const dyd_scan *scan);            /* [n_cells] */
int32_t dyd_scan_parts(const dyd_scan *scan);
int dyd_scan_part(const dyd_scan *scan, int32_t k, int64_t *lo, int64_t *hi, const uint8_t **text, const int64_t **off);
int dyd_scan_text(dyd_scan *scan, const uint8_t **text, const int64_t **off);
void dyd_scan_totals(const dyd_scan *scan, int64_t *counts3, double *seconds3);   /* boxes, points, fast-lane cells | scan, device, emit s */
void dyd_scan_free(dyd_scan *scan);
/* measurement / test aid (host, multithreaded): the annotation cells of a synthetic table as json.dumps would write them
 * (deal-yolo-daya_amd/synth.py: row_json) — flat utf-8 in *out_text (release with dyd_host_free) and offsets [n_rows+1]. */
int dyd_synth_json(const double *xy, const int32_t *pt_off, const int32_t *box_off, const int32_t *label, const uint8_t *int_row,
                   int64_t n_rows, int64_t width, int64_t height, int n_threads, uint8_t **out_text, int64_t *out_off);

/* ---- native expansion of the split step (HOST code, multithreaded) -----------------------------------
 * Replaces the per-row Python of split_dataset_by_rules (processor.py:712-792; utils.py:645-662): every row
 * becomes one record per (object, label of the object's name found in the rules), the record's JSON being the
 * row's document with "objects" reduced to that object and its "name" set to the label (:760-767).
 * text/cell_off/missing: the rows' JSON cells (missing = no usable cell: "空数据"); label_text/label_off: the
 * keys of label_to_category.  Per cell: status (0 expanded, 1 空数据, 2 JSON解析失败, 3 objects不是列表,
 * 4 标注字段objects为空, 5 irregular: the Python path decides), number of records, the label combination
 * ("，".join(sorted(labels)), :736) and the joined reasons ("；".join(sorted(标签…未在规则中定义)), :779).
 * Records in row order: cell index, label index, JSON text.  Events in the order the reference appends to its
 * unclassified list: cell index, kind (1 标注框缺少name字段, 2 label not in the rules, 3 nothing classified),
 * the label for kind 2. */
typedef struct dyd_split dyd_split;
int dyd_json_split_expand(const uint8_t *text, const int64_t *cell_off, const uint8_t *missing, int64_t n_cells,
                          const uint8_t *label_text, const int64_t *label_off, int32_t n_labels, int n_threads,
                          dyd_split **out);
const uint8_t *dyd_split_status(const dyd_split *h);          /* [n_cells] */
const int32_t *dyd_split_n_expanded(const dyd_split *h);      /* [n_cells] */
int64_t dyd_split_rows(const dyd_split *h);
const int64_t *dyd_split_row_cell(const dyd_split *h);        /* [rows] */
const int32_t *dyd_split_row_label(const dyd_split *h);       /* [rows] */
int64_t dyd_split_events(const dyd_split *h);
const int64_t *dyd_split_event_cell(const dyd_split *h);      /* [events] */
const uint8_t *dyd_split_event_kind(const dyd_split *h);      /* [events] */
/* which: 0 record JSON [rows] (a flat copy, made on the first request), 1 label combination [n_cells], 2 joined reasons
 * [n_cells], 3 event label [events] (made on the first request), 4 the distinct undefined labels [dyd_split_undefined] */
int dyd_split_strings(dyd_split *h, int which, const uint8_t **data, const int64_t **off);
/* the same expansion over one (pointer, length) view per cell — the str objects of a DataFrame column, nothing copied */
int dyd_json_split_expand_v(const uint8_t *const *cell_ptr, const int64_t *cell_len, const uint8_t *missing, int64_t n_cells,
                            const uint8_t *label_text, const int64_t *label_off, int32_t n_labels, int n_threads,
                            dyd_split **out);
/* table-scale accessors: the record texts stay in the worker threads' buffers, one (address, length) view per record in row
 * order (valid until dyd_split_free); an event of kind 2 carries the index of its label in the table of distinct undefined
 * labels (-1 otherwise); per label of the rules the first record carrying it (-1: none) and its number of records — the
 * first-appearance order of the categories (processor.py:773) without a pass over the records */
int dyd_split_rec_views(const dyd_split *h, const uint64_t **ptr, const int64_t **len);
const int32_t *dyd_split_event_code(const dyd_split *h);      /* [events] */
int64_t dyd_split_undefined(const dyd_split *h);
const int64_t *dyd_split_label_first(const dyd_split *h);     /* [n_labels] */
const int64_t *dyd_split_label_count(const dyd_split *h);     /* [n_labels] */
int64_t dyd_split_fast_cells(const dyd_split *h);             /* cells the single-parse lane took */
int dyd_split_all_ascii(const dyd_split *h);                  /* 1: every record text is pure ASCII */
/* The reasons of a table are few distinct texts (they name a row's undefined labels): per cell the index of its text among the
 * distinct ones (-1: no reasons), or NULL when there were more than 4096 of them; their number; per distinct text the first cell
 * carrying it (its bytes are dyd_split_strings(h, 2) at that cell). */
const int32_t *dyd_split_reason_code(const dyd_split *h);
int64_t dyd_split_reason_distinct(const dyd_split *h);
const int64_t *dyd_split_reason_first(const dyd_split *h);
void dyd_split_seconds(const dyd_split *h, double *parse_gather2);
void dyd_split_free(dyd_split *h);

/* ---- native relabelling of the label_replace step (HOST code, multithreaded) ------------------------------
 * Replaces the per-row Python of replace_labels_by_mapping (processor.py:565-609; utils.py:659-679): in every
 * document whose "objects" is a list, the name of each dict element is split into labels, the labels found among
 * the keys are replaced, the result de-duplicated, sorted and joined with ","; the whole document is re-serialised
 * as json.dumps(..., ensure_ascii=False) does.  key_text/key_off, val_text/val_off: the old -> new label pairs.
 * Per cell: status (0 rewritten, 1 skipped: no usable cell, 2 JSON decode error, 3 left as it is: "objects" absent
 * or not a list, 5 irregular: the Python path decides), five counters (objects, names missing, labels seen, labels
 * replaced, objects renamed), whether some name would change, and for those the old / new names joined with "；"
 * (:605-609).  The labels that are not keys of the mapping, in order of appearance, with their cell. */
typedef struct dyd_relabel dyd_relabel;
int dyd_json_relabel(const uint8_t *text, const int64_t *cell_off, const uint8_t *missing, int64_t n_cells,
                     const uint8_t *key_text, const int64_t *key_off, const uint8_t *val_text, const int64_t *val_off,
                     int32_t n_pairs, int n_threads, dyd_relabel **out);
const uint8_t *dyd_relabel_status(const dyd_relabel *h);        /* [n_cells] */
const uint8_t *dyd_relabel_has_diff(const dyd_relabel *h);      /* [n_cells] */
const int32_t *dyd_relabel_counts(const dyd_relabel *h);        /* [n_cells][5] */
int64_t dyd_relabel_tokens(const dyd_relabel *h);
const int64_t *dyd_relabel_token_cell(const dyd_relabel *h);    /* [tokens] */
/* which: 0 text after the step [n_cells] (the cell itself unless status 0; empty for status 1), 1 joined old names [n_cells], 2 joined new names [n_cells], 3 unmatched label [tokens] */
int dyd_relabel_strings(const dyd_relabel *h, int which, const uint8_t **data, const int64_t **off);
void dyd_relabel_free(dyd_relabel *h);

/* ---- native CSV hand-off (HOST code) ------------------------------------------------
 * Replaces pandas read_csv / to_csv around the two heavy JSON columns (processor.py:235, :309, :379,
 * :404, :407).  dyd_csv_index tokenises a utf-8 buffer with pandas' C-parser conventions and FAILS on
 * anything it does not reproduce exactly (the caller then uses pandas); dyd_csv_extract returns one
 * column as flat utf-8 + offsets + a per-cell class (0 text, 1 missing = one of pandas' default NA strings,
 * 2 text that dtype inference could read as a number / boolean); dyd_csv_project returns CSV text
 * of the same width in which only the `keep` columns carry their cells, for pandas itself to parse with
 * usecols (same width => same low-memory piece boundaries => same per-piece dtype inference as on the
 * original file); dyd_csv_write writes typed column buffers
 * (kind 0 utf-8, 1 int64, 2 float64, 3 bool) like DataFrame.to_csv(index=False). */
typedef struct dyd_csv dyd_csv;
typedef struct dyd_csv_col {
    int32_t kind;
    const void *data;
    const int64_t *off;
    const uint8_t *na;
} dyd_csv_col;
int dyd_csv_index(const uint8_t *text, int64_t len, dyd_csv **out);
int64_t dyd_csv_rows(const dyd_csv *csv);
int32_t dyd_csv_cols(const dyd_csv *csv);
int64_t dyd_csv_header(const dyd_csv *csv, int32_t col, uint8_t *buf, int64_t cap);
int dyd_csv_extract(dyd_csv *csv, int32_t col, const uint8_t **bytes, const int64_t **off, const uint8_t **na);
int dyd_csv_project(dyd_csv *csv, const int32_t *keep, int32_t n_keep, const uint8_t **text, int64_t *len);
int64_t dyd_csv_col_bytes(const dyd_csv *csv, int32_t col);   /* total cell bytes of a column */
int64_t dyd_csv_row_end(const dyd_csv *csv, int64_t row);     /* byte offset behind data row `row` (-1: the header) */
int dyd_csv_has_cr(const dyd_csv *csv);                       /* 1: some lines end with "\r\n" */
void dyd_csv_free(dyd_csv *csv);
/* mode 0: write `path` anew, 1: to memory (*mem_out, dyd_host_free), 2: append to `path` (merge step, :73-76) */
int dyd_csv_write(const char *path, const uint8_t *header, int64_t header_len, const dyd_csv_col *cols,
                  int32_t n_cols, int64_t n_rows, const int64_t *rows, int64_t n_sel, int quote_cr,
                  int n_threads, int mode, uint8_t **mem_out, int64_t *mem_len);
void dyd_host_free(void *p);

/* ---- tuning hook (not reference-facing): selects kernel variants for A/B measurement,
 * e.g. dyd_set_option("k1_variant", 1) = K1 without LDS staging; "k7_variant": -1 by the table's shape (default),
 * 2 / 22 row tiles (one / two per ticket), 30 box tiles (rows of many boxes); "fused_variant": -1 by the table's shape (default:
 * 4 up to 32 boxes per image on average, 10 beyond, 6 / 9 for polygons of 20..48 points), 4 = wave kernel, 10 = its dense
 * instantiation (rows of 40..256 boxes sorted and swept), 6 / 9 = workgroup tilings, 1 = two launches;
 * "k2_variant": -1 by shape, 4 = the wave kernel's pair stage, 0..3 / 5 = tile kernels (2 / 3 / 5 with the f32 filter and the sweep);
 * "k14_lane_edges": the largest number of edges of U whose self-intersection test K14 runs in one lane (<= 0: the default);
 * "k19_lane_points": the largest polygon (points) K19 simplifies in one lane (default 32, at most 64), "k19_lds_points": the
 * largest one a workgroup stages in LDS (default and at most 1024; beyond it the points stream from HBM); <= 0: the default;
 * "k21_strip" / "k21_crossings" and "k22_strip" / "k22_crossings": the strip width (default and at most 1024) and the capacity of
 * the crossing list (256) of K21 and of K22, "k22_chunk": the B bitmaps K22 holds at a time (32), "k22_grid": a cap on K22's paint
 * workgroups (2^20); "k23_strip" / "k23_band" / "k23_crossings" / "k23_grid": K23's strip width (default and at most 1024), the
 * scanlines per band (default 64), the capacity of its crossing list (256) and a cap on its walk workgroups (2^20); <= 0: the
 * default, larger values are capped. */
int dyd_set_option(const char *key, int64_t value);
/* measurement aid: plain streaming kernel (mode 0 copy, 1 read-only, 2 write-only, 3-5 the same non-temporal, 16 B per
 * lane) used to record the box's HBM ceiling next to the kernels' achieved GB/s; modes 6 / 7 / 8: one 8-byte word per lane
 * at a pseudo-random place of `dst` (scatter / gather / atomicMin, every word once) — the ceiling K4/K5/K6 are quoted against;
 * modes 10 / 11 / 12: the fused kernel's 72 % read / 28 % write mix (five 16-byte loads in flight per lane, two 16-byte stores;
 * plain, non-temporal stores, non-temporal both): `bytes` of src are read, 2/5 of that written to dst. */
int dyd_membench_dev(int mode, const void *src, void *dst, int64_t bytes, int blocks, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DYD_H */
