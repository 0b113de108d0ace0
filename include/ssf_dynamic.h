/*
 * ssf_dynamic.h -- per-pixel dynamic-object masks, voted onto the superpixels of the frame on the device.
 *
 * The dynamic_mask argument of ssf.h takes one byte per SUPERPIXEL of the frame being submitted, but the superpixels of a
 * frame exist only once the library has segmented it, inside the very call that takes the mask.  What a motion detector,
 * a person detector or a segmenter produces is a mask in image coordinates.  The entry points below take that instead.
 *
 * A pixel mask is H*W bytes, row-major with stride W.  A non-zero byte means the pixel shows a moving object.  For a frame
 * submitted with a pixel mask:
 *   - label is the frame's final label map: what ssf_get_index_map returns, after the last relabelling pass.
 *   - total[s] = number of pixels with label == s.  masked[s] = number of those pixels whose mask byte is non-zero.
 *   - Superpixel s is dynamic iff masked[s] > 0 && 2 * masked[s] >= total[s]: at least half of its pixels are masked.
 *     The arithmetic is integer, so the decision is exact.
 *   - A dynamic superpixel gets frame confidence -1.  This is exactly what the one-byte-per-superpixel dynamic_mask of ssf.h
 *     does, so ICP, association, insertion and classification treat it as invalid.
 *   - Nothing else changes.  The label map, inlier map, plane depth, superpixel table and the free-space test of the
 *     classification stay as they are.
 *
 * The reference's own rule (its motion detection and YOLO person boxes mark superpixels inside processFrame) cannot be pinned
 * here: its source is not on hand.  The majority vote above is this library's specification.  There is no threshold
 * parameter: a caller who wants "any masked pixel" or "centroid inside the box" shapes the mask itself.
 *
 * The counts are taken by the kernel that already reads the final label map of every tile (k_render_moments), with integer
 * atomics over a partition of the image: exact and independent of scheduling.  Frames and batches without a pixel mask run
 * the very kernels they run without this header.
 *
 * Arguments:
 *   pixel_mask    NULL = no mask: then the call is identical, bit for bit and in the kernels it launches, to the ssf.h call
 *                 without a dynamic_mask.  A host pointer, or a device pointer when on_device is set; device masks need no
 *                 alignment.  It must stay valid and unmodified as long as the frame buffers of the same call (ssf.h,
 *                 ssf_submit_frame).
 *   on_device     as ssf_submit_frame: rgb, depth and pixel_mask are device pointers.
 *   pixel_masks   ssf_process_sequence_pixmask: NULL (no masks at all) or n entries, each of which may be NULL.
 * The frame pointers are read in the handle's input format (ssf_input.h).  These calls take no S-byte dynamic_mask; the ssf.h
 * calls keep theirs, unchanged.  Refused like the ssf.h calls: a NULL handle or frame pointer (SSF_ERR_INVALID_ARG), a full
 * pipeline or pending frames where ssf.h refuses them (SSF_ERR_STATE), a device frame not aligned for the input format.
 *
 * ssf_get_dynamic_superpixels: the vote of the last processed (or stage-extracted) frame: S bytes, 1 = dynamic by the pixel
 * mask, 0 otherwise (all 0 when that frame had no pixel mask); *n_dynamic (nullable) = their number.  It does not include the
 * superpixels that are invalid for other reasons.  Valid as long as the other per-frame getters of ssf.h (ssf_get_index_map).
 * With the extract stage dealt over the ranks (ssf_comm_deal_extract) the vote is reported by the rank that extracted the
 * frame; the others receive its confidences.
 *
 * Only the HIP product library (libssf_hip.so) exports these functions; the ABI version of ssf.h is unchanged.
 */
#ifndef SSF_DYNAMIC_H
#define SSF_DYNAMIC_H

#include "ssf.h"

#ifdef __cplusplus
extern "C" {
#endif

int ssf_process_frame_pixmask(ssf_handle* h, const void* rgb, const void* depth, int on_device,
                              const float* prior_pose, const uint8_t* pixel_mask, ssf_frame_result* out);
int ssf_submit_frame_pixmask(ssf_handle* h, const void* rgb, const void* depth, int on_device, const uint8_t* pixel_mask);
int ssf_process_sequence_pixmask(ssf_handle* h, const void* const* rgb, const void* const* depth,
                                 const uint8_t* const* pixel_masks, int n, int on_device, ssf_frame_result* out);
int ssf_stage_extract_pixmask(ssf_handle* h, const void* rgb, const void* depth, int on_device, const uint8_t* pixel_mask);
int ssf_get_dynamic_superpixels(ssf_handle* h, uint8_t* out, int* n_dynamic);

#ifdef __cplusplus
}
#endif

#endif /* SSF_DYNAMIC_H */
