/*
 * ssf_input.h -- input frame formats of a handle (raw sensor frames).
 *
 * By default every frame entry point of ssf.h reads colour as H*W*3 bytes in RGB order and depth as H*W
 * float32 metres.  A handle can be told once to read frames as an RGB-D sensor delivers them instead:
 *
 *   colour  SSF_COLOR_RGB8 (default) | SSF_COLOR_BGR8   H*W*3 bytes
 *           SSF_COLOR_RGBA8 | SSF_COLOR_BGRA8           H*W*4 bytes, the alpha byte is ignored
 *   depth   SSF_DEPTH_F32_METRES (default)              H*W float32 metres
 *           SSF_DEPTH_U16_SCALED                        H*W uint16 counts; the depth used is
 *                                                       (float)((double)v * depth_scale) metres
 *                                                       (depth_scale: metres per count, 0.0002 for TUM;
 *                                                       0 counts = 0 m = a hole)
 *
 * The conversion is done by the kernels that load the pixels (no extra launch, no intermediate buffer) and is the
 * one the reference's nodes apply on the host (convertTo(CV_32FC1, depthScale), cvtColor): results are bit-identical
 * to feeding the converted frame in the default format.
 *
 * After ssf_set_input_format, ssf_process_frame, ssf_process_frame_device, ssf_submit_frame, ssf_process_sequence,
 * ssf_stage_extract and ssf_bilateral_filter (its input; the output stays float32 metres) read their frame pointers
 * in that format.  Device pointers must be aligned for it: 2 bytes for uint16 depth, 4 bytes for 4-byte colour
 * (SSF_ERR_INVALID_ARG otherwise).  ssf_fern_codes keeps its own arguments.
 *
 * ssf_set_input_format returns SSF_ERR_INVALID_ARG for an unknown enum value or, with SSF_DEPTH_U16_SCALED, a
 * depth_scale that is not finite and > 0 (with SSF_DEPTH_F32_METRES the scale is ignored and reported as 1.0), and
 * SSF_ERR_STATE while frames are pending (ssf_pending_frames() > 0) or a sequence is being processed.
 *
 * Only the HIP product library (libssf_hip.so) exports these functions; the ABI version of ssf.h is unchanged.
 */
#ifndef SSF_INPUT_H
#define SSF_INPUT_H

#include "ssf.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef enum ssf_color_format {
    SSF_COLOR_RGB8 = 0,
    SSF_COLOR_BGR8 = 1,
    SSF_COLOR_RGBA8 = 2,
    SSF_COLOR_BGRA8 = 3
} ssf_color_format;

typedef enum ssf_depth_format {
    SSF_DEPTH_F32_METRES = 0,
    SSF_DEPTH_U16_SCALED = 1
} ssf_depth_format;

int ssf_set_input_format(ssf_handle* h, int color_format, int depth_format, double depth_scale);
int ssf_get_input_format(const ssf_handle* h, int* color_format, int* depth_format, double* depth_scale);

#ifdef __cplusplus
}
#endif

#endif /* SSF_INPUT_H */
