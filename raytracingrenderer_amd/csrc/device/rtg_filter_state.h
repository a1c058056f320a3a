// rtg_filter_state.h — the host layer shared by the film-filter units: the denoiser (rtg_denoise.hip), the
// temporal unit (rtg_temporal.hip), the variance-guided chain that joins them (rtg_svgf.hip), its illumination
// mode (rtg_svgf_illum.hip) and the fused first-hit pass that feeds them (rtg_gbuffer.hip). Their states own their device memory (DevBuf) and their
// timing events (DevEvents), so releasing one is `delete`; each is built as a local object and handed to the
// handle only once every allocation has succeeded, so the handle never holds a half-built
// one. No kernel and no device function lives here: the two temporal kernels share rtg_reproject.h, every
// other kernel is its unit's own.
#pragma once
#include "rtg_internal.h"

#include <cstring>
#include <memory>

struct TemporalProj {  // the history camera's projectOntoCamera state
    float P[16];       // projectionMatrix
    float C2V[16];     // cameraToView
    float W, H;
};

struct SvgfState {  // rtg_svgf.hip's part of the temporal state
    DevBuf<float2> mom[2];                  // mom[cur] is M = {mu1, mu2}, the ping-pong partner of hist
    int cur = 0;
    bool mom_valid = false;                 // M belongs to H (cleared by rtg_temporal_accumulate)
    bool have_result = false;
    DevBuf<float4> col[2];                  // {rgb, v}, the filter's ping-pong
    DevBuf<float> var;                      // the variance fed to level 0
    DevBuf<float4> xpos;                    // the current guide's {X, t} halves, packed for the filter's taps
    DevBuf<float> out;                      // last result, tightly packed rgb
    DevEvents<8> ev;
    double guide_ms = 0.0, accumulate_ms = 0.0, variance_ms = 0.0, filter_ms = 0.0;
};

struct HistoryTrack {  // a history with the camera it was seen from and that camera's guide
    DevBuf<float4> hist[2];                 // hist[cur] is H
    int cur = 0;
    DevBuf<float4> hguide;                  // the history camera's guide (valid when have_hist)
    bool have_hist = false;
    DevCamera hcam{};
    rtg_camera_proj hproj{};
};

struct SvgfIllumState {  // rtg_svgf_illum.hip's part: the illumination mode's own history, moments and guide
    HistoryTrack k;                         // H' (illumination), its camera and its classed guide
    SvgfState sv;                           // M', the filter's buffers, the last result
    DevBuf<float> film;                     // F', the film's sums over the divisor
    DevBuf<float4> guide;                   // G', the current camera's classed guide (swapped with k.hguide)
    double prepare_ms = 0.0, unpack_ms = 0.0;
};

struct TemporalState : HistoryTrack {
    size_t n = 0;                           // pixels the buffers hold
    DevBuf<float4> cguide;                  // the guide cache (valid for ccam / cproj when cache_ready)
    DevBuf<float> out;                      // last result, tightly packed rgb
    bool cache_ready = false, have_result = false;
    DevCamera ccam{};
    rtg_camera_proj cproj{};
    DevEvents<4> ev;
    double guide_ms = 0.0, accumulate_ms = 0.0;
    double gbuffer_ms = 0.0;                // the fused pass of the last rtg_gbuffer / rtg_svgf_accumulate (0: none ran)
    std::unique_ptr<SvgfState> sv;          // built by the first rtg_svgf_accumulate
    std::unique_ptr<SvgfIllumState> il;     // built by the first rtg_svgf_illum_accumulate
};

struct DenoiseState {
    size_t n = 0;                  // pixels the buffers hold
    DevBuf<float4> col[2];
    DevBuf<float4> guide;          // packed guides (valid when guides_ready)
    DevBuf<float> albedo;          // the guide films as rendered (rtg_denoise_guides)
    DevBuf<float> normal;
    DevBuf<float> out;             // last result, tightly packed rgb
    bool guides_ready = false, have_result = false;
    DevEvents<2> ev;               // (none in rtg_denoise_images' local state)
    double ms = 0.0;
};

// device time from event a to event b of a stage that ran and has finished; 0 for one that did not run
static inline double stage_ms(bool ran, hipEvent_t a, hipEvent_t b) {
    float ms = 0.0f;
    return (ran && hipEventElapsedTime(&ms, a, b) == hipSuccess) ? ms : 0.0;
}

// rtg_temporal.hip
// RTG_ERR_ARG ("who: <what> must be ...") for a size outside 1..65535 per side or above 2^28 pixels
int check_size(const char* who, int64_t W, int64_t H, const char* what = "the film");
// the handle's temporal state, built on first use (RTG_ERR_ARG for a film check_size refuses)
int temporal_state(const char* who, rtg_handle* h);
// RTG_ERR_ARG (with "who: ..." as the message) for parameters outside include/rtg.h's ranges
int temporal_check(const char* who, const rtg_temporal_params* p);
bool same_camera(const DevCamera& a, const rtg_camera_proj& ap, const DevCamera& b, const rtg_camera_proj& bp);
// the guide of the handle's camera, queued on h's stream; with_denoiser: the denoiser's guides with it, by one
// fused first-hit pass when either is missing (see its definition)
int current_guide(rtg_handle* h, bool with_denoiser, const float4** guide, bool* traced);
// a guide's W * H records downloaded, their halves split into the caller's two images (either may be null)
int download_guide(const rtg_handle* h, const float4* guide, float* pos_t, float* normal_id);
// after an accumulate whose result is complete: hist flips, and unless the camera was the history's, the
// stored camera and guide (g, as current_guide gave it) become the current ones
void temporal_advance(rtg_handle* h, bool unchanged, const float4* g);
// A unit's last result (W * H rgb on the device, null: none yet, refused as "who: <none>") copied to device
// memory on h's stream, and waited for
int copy_result(const char* who, rtg_handle* h, const float* result, void* dst_device, const char* none = "no result yet");
// rtg_denoise.hip
// the handle's denoiser state, built on first use
int denoise_state(rtg_handle* h);
// the albedo / shading-normal guides, rendered and packed when dropped; wait: the host waits for them
int ensure_guides(rtg_handle* h, bool wait = true);
// rtg_svgf.hip
// RTG_ERR_ARG (with "who: ..." as the message) for parameters outside include/rtg.h's ranges
int svgf_check(const char* who, const rtg_svgf_params* p);
// the buffers and events of a variance-guided state for n pixels
int svgf_alloc(SvgfState& s, size_t n);
// One step of the chain queued on h's stream with no host wait: k_svgf_temporal on `film` over the history k and
// the moments of s, k_svgf_variance, the copy of the positions and the levels, with g the current camera's
// geometry guide (k's own when the camera is k's: *unchanged). Records s.ev[2..5]; the last level's records are
// s.col[p->iterations & 1]. Nothing of k or s is advanced: svgf_done does that once the stream has been waited for.
int svgf_queue(rtg_handle* h, const rtg_svgf_params* p, const HistoryTrack& k, SvgfState& s, const float* film,
               const float4* g, bool* unchanged);
// after the wait: the stage times (the guide pass ran: traced), M flips and the state holds a result
void svgf_done(SvgfState& s, bool traced);
// rtg_gbuffer.hip: k_gbuffer on st, from the first hits in pb into geo (2 records per pixel) and d's three
// guide buffers
int launch_gbuffer(rtg_handle* h, const PathBufs& pb, float4* geo, DenoiseState& d, hipStream_t st);

// One temporal step's set-up, for TemporalArgs and SvgfTemporalArgs alike: whether the camera is the history's
// (returned), the mode that follows, and every field the two kernels share but gcur, which the caller sets in
// mode 2 once it has the current guide.
template <class Args>
static inline bool temporal_setup(const rtg_handle* h, const HistoryTrack& t, const rtg_temporal_params& p, Args& a) {
    const bool unchanged = t.have_hist && same_camera(h->cam, h->proj, t.hcam, t.hproj);
    a.film = h->d_film;
    a.m = (float)h->spp;
    a.mode = !t.have_hist ? 0 : (unchanged ? 1 : 2);
    a.hin = t.hist[t.cur].p;
    a.hout = t.hist[t.cur ^ 1].p;
    a.W = h->W;
    a.H = h->H;
    a.max_history = p.max_history;
    a.plane_tolerance = p.plane_tolerance;
    a.normal_cos = p.normal_cos;
    if (a.mode == 2) {
        a.ghist = t.hguide.p;
        std::memcpy(a.cam.P, t.hproj.proj, sizeof(a.cam.P));
        std::memcpy(a.cam.C2V, t.hproj.camera_to_view, sizeof(a.cam.C2V));
        a.cam.W = t.hcam.width;
        a.cam.H = t.hcam.height;
    }
    return unchanged;
}
