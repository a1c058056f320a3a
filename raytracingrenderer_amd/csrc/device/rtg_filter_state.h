// rtg_filter_state.h — host-only declarations shared by the film-filter units: the denoiser
// (rtg_denoise.hip), the temporal unit (rtg_temporal.hip) and the variance-guided chain that joins them
// (rtg_svgf.hip), and the fused first-hit pass that feeds them (rtg_gbuffer.hip). No kernel and no device
// function lives here: each unit keeps its own.
#pragma once
#include "rtg_internal.h"

struct TemporalProj {  // the history camera's projectOntoCamera state
    float P[16];       // projectionMatrix
    float C2V[16];     // cameraToView
    float W, H;
};

struct SvgfState;  // rtg_svgf.hip's buffers, below

struct TemporalState {
    size_t n = 0;                           // pixels the buffers hold
    float4* hist[2] = {nullptr, nullptr};   // hist[cur] is H
    int cur = 0;
    float4* hguide = nullptr;               // the history camera's guide (valid when have_hist)
    float4* cguide = nullptr;               // the guide cache (valid for ccam / cproj when cache_ready)
    float* out = nullptr;                   // last result, tightly packed rgb
    bool have_hist = false, cache_ready = false, have_result = false;
    DevCamera hcam{}, ccam{};
    rtg_camera_proj hproj{}, cproj{};
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    double guide_ms = 0.0, accumulate_ms = 0.0;
    double gbuffer_ms = 0.0;                // the fused pass of the last rtg_gbuffer / rtg_svgf_accumulate (0: none ran)
    SvgfState* sv = nullptr;                // allocated by the first rtg_svgf_accumulate
};

struct SvgfState {
    float2* mom[2] = {nullptr, nullptr};    // mom[cur] is M = {mu1, mu2}, the ping-pong partner of hist
    int cur = 0;
    bool mom_valid = false;                 // M belongs to H (cleared by rtg_temporal_accumulate)
    bool have_result = false;
    float4* col[2] = {nullptr, nullptr};    // {rgb, v}, the filter's ping-pong
    float* var = nullptr;                   // the variance fed to level 0
    float4* xpos = nullptr;                 // the current guide's {X, t} halves, packed for the filter's taps
    float* out = nullptr;                   // last result, tightly packed rgb
    hipEvent_t ev[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    double guide_ms = 0.0, accumulate_ms = 0.0, variance_ms = 0.0, filter_ms = 0.0;
};

struct DenoiseState {
    size_t n = 0;                  // pixels the buffers hold
    float4* col[2] = {nullptr, nullptr};
    float4* guide = nullptr;       // packed guides (valid when guides_ready)
    float* albedo = nullptr;       // the guide films as rendered (rtg_denoise_guides)
    float* normal = nullptr;
    float* out = nullptr;          // last result, tightly packed rgb
    bool guides_ready = false, have_result = false;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    double ms = 0.0;
};

// rtg_temporal.hip
// the handle's temporal state, allocated on first use (RTG_ERR_ARG for a film outside 1..65535 per side)
int temporal_state(const char* who, rtg_handle* h);
// RTG_ERR_ARG (with "who: ..." as the message) for parameters outside include/rtg.h's ranges
int temporal_check(const char* who, const rtg_temporal_params* p);
bool same_camera(const DevCamera& a, const rtg_camera_proj& ap, const DevCamera& b, const rtg_camera_proj& bp);
// the guide of the handle's camera, queued on h's stream (see its definition)
int current_guide(rtg_handle* h, const float4** guide, bool* traced);
// ... and the denoiser's guides with it, by one fused first-hit pass when either is missing (see its definition)
int current_gbuffer(rtg_handle* h, const float4** guide, bool* traced);
// after an accumulate whose result is complete: hist flips, and unless the camera was the history's, the
// stored camera and guide (g, as current_guide gave it) become the current ones
void temporal_advance(rtg_handle* h, bool unchanged, const float4* g);
// rtg_denoise.hip
// the handle's denoiser state, allocated on first use
int denoise_state(rtg_handle* h);
// the albedo / shading-normal guides, rendered and packed when dropped; wait: the host waits for them
int ensure_guides(rtg_handle* h, bool wait = true);
// rtg_gbuffer.hip: k_gbuffer on st, from the first hits in pb into geo (2 records per pixel) and d's three
// guide buffers
int launch_gbuffer(rtg_handle* h, const PathBufs& pb, float4* geo, DenoiseState& d, hipStream_t st);
// rtg_svgf.hip: frees t.sv (temporal_release)
void svgf_release(TemporalState& t);
