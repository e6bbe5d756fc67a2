/*
 * ocvar_multi_format.h -- the input format of an OcvarMulti (included by ocvar_multi.h; its own file so that the list of
 * entry points ocvar_multi.h itself declares stays that of the multi-GPU batch and tracking calls).
 */
#ifndef OCVAR_MULTI_FORMAT_H
#define OCVAR_MULTI_FORMAT_H

#include "ocvar_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct OcvarMulti OcvarMulti;

/* ocvar_hip_set_input_format on every device's context: what the frames of the ocvar_multi_detect_* / ocvar_multi_track_*
 * calls hold (OCVAR_FMT_*, default OCVAR_FMT_BGR; row_stride at least bytes per pixel times width).  OCVAR_E_ARG for an unknown
 * format. */
int ocvar_multi_set_input_format(OcvarMulti* m, int format);
/* ocvar_hip_set_corner_refine on every device's context (half_win 0 = off, the default).  OCVAR_E_ARG outside its ranges. */
int ocvar_multi_set_corner_refine(OcvarMulti* m, int half_win, int max_iter, float eps);

#ifdef __cplusplus
}
#endif
#endif
