// sddc_ddc_internal.h — development-only entry points (not part of the C ABI contract).
#pragma once
#include "sddc_ddc.h"
#ifdef __cplusplus
extern "C" {
#endif
/* A tuning parameter of the kernels (A/B timing, tools/ab_libs.py --param):
 * SDDC_DDC_PARAM_FS_STATIC_PCT = the d = 0 kernel's share of each workgroup's frames taken
 * statically before it draws from the dynamic queue (0..100, default kFsStaticPct). */
#define SDDC_DDC_PARAM_FS_STATIC_PCT 1
/* SDDC_DDC_PARAM_SLOT_WEIGHTS = 1: the persistent kernel splits the frames by CU slot speed
 * (kSlotWeights[d]), 0: equal contiguous ranges (default kSlotWeighting). */
#define SDDC_DDC_PARAM_SLOT_WEIGHTS 2
/* SDDC_DDC_PARAM_FS_FRAMES_PER_WG = n > 0: the d = 0 kernel runs a non-persistent grid of
 * ceil(frames / n) workgroups, n frames each, balanced by the hardware dispatcher; 0 (default):
 * the persistent grid. */
#define SDDC_DDC_PARAM_FS_FRAMES_PER_WG 3
/* SDDC_DDC_PARAM_FS_SCHEDULE: the d = 0 kernel's frame schedule, 0 = the slot-weighted static
 * split alone (default), 1 = static prefix + dynamic queue, 2 = work stealing (1 and 2 only for
 * CF32 output without NCO, rand or sideband inversion; other configurations fail to launch). */
#define SDDC_DDC_PARAM_FS_SCHEDULE 4
/* SDDC_DDC_PARAM_FS_STEAL_MINREM: a thief steals only from ranges with at least this many
 * unclaimed frames (1..64; 0: no stealing, the static split inside the stealing kernel). */
#define SDDC_DDC_PARAM_FS_STEAL_MINREM 5
/* SDDC_DDC_PARAM_FS_STEAL_PUBLIC: frames at the end of each workgroup's range open to thieves,
 * claimed by the owner with atomics (0: all but the first two); the rest the owner takes alone. */
#define SDDC_DDC_PARAM_FS_STEAL_PUBLIC 6
/* SDDC_DDC_PARAM_FS_ZERO_ROWS != 0 (default 1): the d = 0 kernel skips the inverse input's whole
 * zero rows of the tune bin (ddc_fs.hip fs_zero_rows: 2..8 rows for CF32 output without the NCO,
 * 4 rows or none for the fused-NCO and CS16 outputs and the queue / stealing schedules; a single
 * zero row is computed); 0: computes them all (A/B, tests). */
#define SDDC_DDC_PARAM_FS_ZERO_ROWS 7
/* SDDC_DDC_PARAM_FS_SLOT_WEIGHTS: the d = 0 kernel's slot weights of the static split, four
 * bytes w0 | w1 << 8 | w2 << 16 | w3 << 24 (CU slot 0 in the low byte, each 1..127); 0: the
 * built-in kFsSlotWeights (A/B of the weights).  Launches with explicit weights use them as they
 * are: the adaptive split (SDDC_DDC_PARAM_FS_ADAPTIVE_SPLIT) neither changes nor measures them. */
#define SDDC_DDC_PARAM_FS_SLOT_WEIGHTS 8
/* SDDC_DDC_PARAM_CH_NCO_RUN_BLOCKS = n > 0: with the per-channel NCO on, process_channels_device
 * cuts a call into runs of at most n input blocks (a chain launch + a channels launch each); 0
 * (default): as many blocks as the lane-start table's byte cap holds (ddc_runtime.cpp
 * kChNcoTableCap), which bounds n > 0 too.  The cut changes no output bit (tests). */
#define SDDC_DDC_PARAM_CH_NCO_RUN_BLOCKS 9
/* SDDC_DDC_PARAM_FS_ADAPTIVE_SPLIT != 0 (default 1): full-residency launches of the d = 0 kernel's
 * static schedule with the built-in slot weights take their per-workgroup frame split from the
 * handle's controller, which learns it from the workgroups' measured start and end times
 * (fs_split_controller.hpp); 0: the built-in slot-weighted split, nothing measured. */
#define SDDC_DDC_PARAM_FS_ADAPTIVE_SPLIT 10
/* SDDC_DDC_PARAM_SPECTRUM_MAX_WGS = n > 0: the spectrum kernel's grid is at most n workgroups, so a
 * workgroup takes several work items and the items outnumber the workgroups; 0 (default): full
 * residency.  The grid changes no output bit (tests). */
#define SDDC_DDC_PARAM_SPECTRUM_MAX_WGS 11
/* SDDC_DDC_PARAM_CHSPEC_MAX_WGS = n > 0: the channel spectrum kernel's grid is at most n workgroups,
 * so a workgroup takes several rounds of work items and the last round is partial; 0 (default):
 * enough workgroups for all items, or full residency with a loop.  The grid changes no output bit
 * (tests). */
#define SDDC_DDC_PARAM_CHSPEC_MAX_WGS 12
/* SDDC_DDC_PARAM_CHDEC_MAX_WGS = n > 0: the channel decimator kernel's grid is at most n workgroups,
 * so a workgroup takes several rounds of (channel, tile) items and the items outnumber the
 * workgroups; 0 (default): one workgroup per item, or full residency with a loop.  The grid changes
 * no output bit (tests). */
#define SDDC_DDC_PARAM_CHDEC_MAX_WGS 13
/* SDDC_DDC_PARAM_CHRES_MAX_WGS = n > 0: the channel resampler kernel's grid is at most n workgroups,
 * as param 13 for the decimator; 0 (default): one workgroup per item, or full residency with a
 * loop.  The grid changes no output bit (tests). */
#define SDDC_DDC_PARAM_CHRES_MAX_WGS 14

/* SDDC_DDC_PARAM_CHDEM_MAX_WGS = n > 0: the channel demodulator kernel's grid is at most n workgroups,
 * as params 13 and 14 for the decimator and the resampler; 0 (default): one workgroup per item, or
 * full residency with a loop.  The grid changes no output bit and no power bit (tests). */
#define SDDC_DDC_PARAM_CHDEM_MAX_WGS 15

/* SDDC_DDC_PARAM_CHAUD_MAX_WGS = n > 0: each of the channel audio filter's three grids is at most n
 * workgroups, as params 13 - 15; 0 (default): one workgroup per wave of items, or full residency with
 * a loop.  The grid changes no output bit and no state bit (tests). */
#define SDDC_DDC_PARAM_CHAUD_MAX_WGS 16

/* SDDC_DDC_PARAM_CHAUD_RUN_BLOCKS = n in 1..2^20: a channel audio filter call is processed in runs of
 * at most n full blocks per channel (plus a head and a tail), which bounds the scratch of a run, as
 * param 9 bounds the NCO table; 0: the default (512).  The run length changes no output bit (tests). */
#define SDDC_DDC_PARAM_CHAUD_RUN_BLOCKS 17

/* SDDC_DDC_PARAM_CHAGC_MAX_WGS = n > 0: each of the channel AGC's three grids is at most n workgroups,
 * as param 16 for the audio filter; 0 (default): one workgroup per wave of items, or full residency
 * with a loop.  The grid changes no output bit, no envelope bit and no state bit (tests). */
#define SDDC_DDC_PARAM_CHAGC_MAX_WGS 18

/* SDDC_DDC_PARAM_CHAGC_RUN_BLOCKS = n in 1..2^20: a channel AGC call is processed in runs of at most
 * n full blocks per channel (plus a head and a tail), which bounds the scratch of a run, as param 17
 * for the audio filter; 0: the default (2048).  The run length changes no output bit (tests). */
#define SDDC_DDC_PARAM_CHAGC_RUN_BLOCKS 19

/* SDDC_DDC_PARAM_LAZY_RECORD != 0 (default 1): a single-channel launch (sddc_ddc_process_device and
 * the host path's launches) notes its stream and records the stream's event only when another
 * stream or the host is about to wait for it; 0: an event record after every launch, as the other
 * entry points do (A/B of the gap between consecutive dispatches). */
#define SDDC_DDC_PARAM_LAZY_RECORD 20

/* SDDC_DDC_PARAM_CHNB_MAX_WGS = n > 0: each of the channel blanker's two grids is at most n workgroups,
 * as param 18 for the AGC; 0 (default): one workgroup per run (or per channel), or full residency with
 * a loop.  The grid changes no output bit and no count (tests). */
#define SDDC_DDC_PARAM_CHNB_MAX_WGS 21

/* SDDC_DDC_PARAM_CHNB_RUN_BLOCKS = n in 1..2^20: a wave of the channel blanker owns n consecutive blocks
 * of a channel (and recomputes what it needs of the blocks before them); 0: chosen from the call's
 * size, 32..128.  The run length changes no output bit and no count (tests). */
#define SDDC_DDC_PARAM_CHNB_RUN_BLOCKS 22

/* SDDC_DDC_PARAM_CHSQ_MAX_WGS = n > 0: each of the channel squelch's three grids is at most n workgroups,
 * as param 21 for the blanker; 0 (default): full residency with a loop.  The grid changes no output bit and
 * no side output (tests). */
#define SDDC_DDC_PARAM_CHSQ_MAX_WGS 23

/* SDDC_DDC_PARAM_CHSQ_RUN_BLOCKS = n in 1..2^20: a call of the channel squelch is cut into launch sets of at
 * most n blocks per channel (the scratch holds one word per channel and block of a set); 0: 4096.  The run
 * length changes no output bit and no side output (tests). */
#define SDDC_DDC_PARAM_CHSQ_RUN_BLOCKS 24

/* SDDC_DDC_PARAM_CHTONE_MAX_WGS = n > 0: each of the channel tone detector's grids is at most n workgroups,
 * as param 23 for the squelch; 0 (default): full residency with a loop.  The grid changes no output bit and
 * no side output (tests). */
#define SDDC_DDC_PARAM_CHTONE_MAX_WGS 25

/* SDDC_DDC_PARAM_CHTONE_RUN_BLOCKS = n in 1..2^20: a call of the channel tone detector is cut into launch
 * sets of at most n blocks per channel, rounded down to whole windows (at least one); 0: 4096.  The run
 * length changes no output bit and no side output (tests). */
#define SDDC_DDC_PARAM_CHTONE_RUN_BLOCKS 26

/* SDDC_DDC_PARAM_CHDCS_MAX_WGS = n > 0: each of the channel DCS decoder's grids is at most n workgroups, as
 * param 25 for the tone detector; 0 (default): full residency with a loop.  The grid changes no output bit
 * and no side output (tests). */
#define SDDC_DDC_PARAM_CHDCS_MAX_WGS 27

/* SDDC_DDC_PARAM_CHDCS_RUN_BLOCKS = n in 1..2^20: a call of the channel DCS decoder is cut into launch sets
 * of at most n blocks per channel, rounded down to whole windows (at least one); 0: 4096.  The run length
 * changes no output bit and no side output (tests). */
#define SDDC_DDC_PARAM_CHDCS_RUN_BLOCKS 28

/* SDDC_DDC_PARAM_CHDCS_BALLOT = 1: the channel DCS decoder's windows kernel forms the sub-bin sums with wave
 * ballots and masked popcounts instead of integer LDS atomics; 0 (default): atomics, the faster route as
 * measured.  Both are sums of the same integers: the route changes no output bit and no side output (tests). */
#define SDDC_DDC_PARAM_CHDCS_BALLOT 29

/* SDDC_DDC_PARAM_CHARS_MAX_WGS = n > 0: the channel audio resampler kernel's grid is at most n
 * workgroups, as param 14 for the resampler; 0 (default): one workgroup per item, or full residency
 * with a loop.  The grid changes no output bit (tests). */
#define SDDC_DDC_PARAM_CHARS_MAX_WGS 30

/* SDDC_DDC_PARAM_CHST_MAX_WGS = n > 0: each of the channel stereo decoder's grids is at most n workgroups, as
 * param 25 for the tone detector; 0 (default): full residency with a loop.  The grid changes no output bit
 * and no side output (tests). */
#define SDDC_DDC_PARAM_CHST_MAX_WGS 31

/* SDDC_DDC_PARAM_CHST_RUN_BLOCKS = n in 1..2^20: a call of the channel stereo decoder is cut into launch sets
 * of at most n blocks per channel (the scratch holds eight words per channel and block of a set); 0: 4096.
 * The run length changes no output bit and no side output (tests). */
#define SDDC_DDC_PARAM_CHST_RUN_BLOCKS 32

int sddc_ddc_internal_set_param(sddc_ddc_t *h, int param, int value);
/* Move the channel stereo decoder's stream position to pos, a multiple of 256 W (SDDC_ERR_ARG otherwise;
 * SDDC_ERR_STATE: no decoder set): the unfinished window's sums and the unfinished block are cleared, the gate,
 * the phase and the last window's results are kept.  It lets tests start a stream next to the 2^32 wrap of the
 * sample phase. */
int sddc_ddc_internal_chst_set_position(sddc_ddc_t *h, uint64_t pos);
/* Move the channel tone detector's stream position to pos, a multiple of 256 W (SDDC_ERR_ARG otherwise;
 * SDDC_ERR_STATE: no detector set): the unfinished window's sums and the unfinished block are cleared, the
 * gate and the last window's results are kept.  It lets tests start a stream next to the 2^32 wrap of the
 * sample phase. */
int sddc_ddc_internal_chtone_set_position(sddc_ddc_t *h, uint64_t pos);
/* A given table of n relative shares (n = the d = 0 kernel's full-residency grid, 4 x CUs) used as
 * it is, without clamps or measurements, until n = 0 clears it (tests). */
int sddc_ddc_internal_fs_set_shares(sddc_ddc_t *h, const float *shares, int n);
/* The adaptive split's state: info[5] = {the controller's grid, measurements used, measurements
 * skipped, the last d = 0 launch took a share table, the last d = 0 launch was measured}; counts
 * receives the current table's frames per workgroup.  Returns the number of counts written. */
int sddc_ddc_internal_fs_split_state(sddc_ddc_t *h, long *info, int *counts, int ncounts);
/* The channel decimator kernel's tile of (factor, ntaps, format): outputs per tile, the polyphase
 * rows' pitch in float2 slots, and the modelled extra LDS cycles of the stage's stores per wave
 * (tools/channel_decimate_banks.py; no handle, no device).  SDDC_ERR_ARG outside the ABI's ranges. */
int sddc_ddc_internal_chdec_layout(int factor, int ntaps, int cs16, int *tile, int *pitch, int *store_conflicts);
/* The channel resampler kernel's tile of (up, down, ntaps, format): outputs per tile (up x the
 * tile's values of a), the polyphase rows' pitch in float2 slots, and the modelled extra LDS cycles
 * of the stage's stores per wave (tools/channel_resample_banks.py; no handle, no device).
 * SDDC_ERR_ARG outside the ABI's ranges. */
int sddc_ddc_internal_chres_layout(int up, int down, int ntaps, int cs16, int *tile_outputs, int *pitch,
                                   int *store_conflicts);
/* Set the resampler's stream position to pos samples consumed (any value: it is kept reduced), the
 * tails left as they are: tests start a stream far out.  SDDC_ERR_STATE: no resampler set. */
int sddc_ddc_internal_chres_set_position(sddc_ddc_t *h, uint64_t pos);
/* The channel audio resampler kernel's tile of (up, down, ntaps, input format): the tile's values of
 * a (up x that many outputs, down x that many samples), the LDS float slots of the kernel instance
 * taken, the polyphase rows' pitch in float slots, and the modelled extra LDS cycles of the stage's
 * stores per wave (no handle, no device).  SDDC_ERR_ARG outside the ABI's ranges. */
int sddc_ddc_internal_chars_layout(int up, int down, int ntaps, int in_s16, int *tile_a, int *lds, int *pitch,
                                   int *store_conflicts);
/* The pitch search of that layout alone: the pitch in [need, max_pitch] for a transposition by mod with
 * V = 4 or 8 samples per lane, and its modelled extra cycles (tools/channel_audio_resample_banks.py is
 * the numpy model it is checked against).  Returns the pitch, or SDDC_ERR_ARG. */
int sddc_ddc_internal_chars_pitch(int mod, int need, int max_pitch, int V, int *store_conflicts);
/* Set the audio resampler's stream position to pos samples consumed (any value: it is kept reduced),
 * the tails left as they are: tests start a stream far out.  SDDC_ERR_STATE: no audio resampler set. */
int sddc_ddc_internal_chars_set_position(sddc_ddc_t *h, uint64_t pos);
/* Set the demodulator's stream position (the index that the BFO phase w * (p + i) counts from), the
 * last samples left as they are: tests start a stream next to the 2^32 wrap.  SDDC_ERR_STATE: no
 * demodulator set. */
int sddc_ddc_internal_chdem_set_position(sddc_ddc_t *h, uint32_t pos);
/* Set the audio filter's stream position (samples since the set; only its value mod
 * SDDC_DDC_AUDIO_BLOCK decides where the blocks end), the states left as they are: tests start a
 * stream inside a block.  SDDC_ERR_STATE: no filter set. */
int sddc_ddc_internal_chaud_set_position(sddc_ddc_t *h, uint64_t pos);
/* Set the AGC's stream position (samples since the set; only its value mod SDDC_DDC_AGC_BLOCK decides
 * where the blocks end), the envelopes left as they are: tests start a stream inside a block.
 * SDDC_ERR_STATE: no AGC set. */
int sddc_ddc_internal_chagc_set_position(sddc_ddc_t *h, uint64_t pos);
/* demod_math.h's two routines as the CPU backend compiles them, on arrays of n values: out[i] =
 * angle(im[i], re[i]); (c[i], s[i]) = cos and sin of 2 pi words[i] / 2^32 (the accuracy sweeps of
 * tests/test_channel_demod_cpu.py; no handle, no device). */
int sddc_ddc_internal_demod_angle(const float *im, const float *re, size_t n, float *out);
int sddc_ddc_internal_demod_sincos(const uint32_t *words, size_t n, float *c, float *s);
/* The controller alone (no handle, no device): tests/test_adaptive_split.py. */
void *sddc_fs_split_create(int G, unsigned slot_weights);
void sddc_fs_split_destroy(void *c);
int sddc_fs_split_load(void *c, const float *shares, int n);
int sddc_fs_split_table(void *c, int ns, unsigned *p, int *first);
int sddc_fs_split_update(void *c, const int *n, const unsigned *start, const unsigned *end);
int sddc_fs_split_model(void *c, double *cost, double *offset);
/* Diagnostic stamp buffers of -DSDDC_STAMPS builds (tools/fs_stamps.py); -1 in product builds. */
int sddc_ddc_internal_fs_stamps(unsigned *host, int nwords, int *words_per_wave);
int sddc_ddc_internal_p_stamps(unsigned *host, int nwords, int *words_per_wave);
#ifdef __cplusplus
}
#endif
