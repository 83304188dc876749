// trsim_train_session.hpp — the training session of a loaded pilot, as its two units see it (trsim_train.hip: the tail, which owns it; trsim_train_conv.hip:
// conv4 .. conv7): the tail's part, the convolutions' part as a member that is empty until trs_pilot_train_convs, how every entry point behind
// trs_pilot_train_begin finds the session, and the one call between the units.  No other unit includes it: the pilot holds the session as the void* it
// hands to trs_train_free (trsim_internal.hpp).
#pragma once
#include <cstdint>
#include <cstring>
#include <memory>

#include "trsim_dropout.hpp"
#include "trsim_internal.hpp"
#include "trsim_mem.hpp"
#include "trsim_train.hpp"
#include "trsim_train_conv.hpp"
#include "trsim_train_dev.hpp"

namespace trsim {

// conv4 .. conv7 of the session (trs_pilot_train_convs)
struct ConvSession {
    uint32_t mask = 0; int lowest = 0, n_cap = 0, cu_count = 0;
    bool held[kConvTrainArrays] = {};       // the master holds this array (trained, or given all the same)
    ConvTrainLayout L{};
    ConvGeom geo[kConvTrainLayers] = {};
    DevBuf<float> master, m, v, g;          // one layout (ConvTrainLayout)
    DevBuf<unsigned short> wt;              // W(l)h as [3][3][CIN][COUT], at the kernels' offsets of the layout: the data-gradient kernel's copy
    DevBuf<float> G, part;                  // G(l) of the layer in hand; the partial sums of the layer in hand (kernel, then bias)
    DevBuf<unsigned short> q[kConvTrainLayers];
    DevBuf<unsigned> scal;                  // [2 j] max |G(l)| bits, [2 j + 1] the exponent s_l (int)
    bool trained(int j) const { return (mask >> j) & 1u; }
};

// dropout behind conv7 (trs_pilot_train_dropout): `on` holds the bits of the sites that drop at all (none at rate 0, where T = 0)
struct DropSession {
    bool called = false;
    uint32_t on = 0, T = 0; float s = 1.0f; uint64_t seed = 0;
    DevBuf<float> act;                    // a'1 | a'2 | a'3, each for n_cap frames: allocated when one of sites 1 .. 3 is on
    bool site(int j) const { return (on >> j) & 1u; }
    bool tail() const { return (on & 0xEu) != 0; }
};

struct TrainSession {
    trs_train_config cfg{};
    DropSession drop;
    int64_t t = 0;
    size_t F = 0; int n_cap = 0, last_n = 0;
    TrainLayout L{};
    DevBuf<float> master, m, v, g;        // one layout (TrainLayout): the eight arrays in order
    DevBuf<float> fwd;                    // out | z1 | z2 | z3 | delta1 | delta2 | delta3 | delta4 (kTrainFrameWidth), each for n_cap frames
    DevBuf<unsigned short> q;             // [n_cap padded to 64][128]
    DevBuf<unsigned> scal;                // [0] max |delta1| bits, [1] the scale's exponent (int), [2] the loss (float)
    std::unique_ptr<ConvSession> conv;    // empty: the convolutions stay as loaded
    // a 28-array session (n_arrays 14): master, m, v and g hold SL's 14 arrays, of which L names the first eight; `side` is fin | y1 | y2 | y3 | delta-y1 |
    // delta-y2 | delta-y3 | fin delta-y1 (kSideFrameWidth), each for n_cap frames
    int n_arrays = kTrainArrays;
    TrainSideLayout SL{};
    DevBuf<float> side;
    bool has_side() const { return n_arrays == kTrainSideArrays; }
    size_t total() const { return has_side() ? SL.off[kTrainSideArrays] : L.off[kTrainArrays]; }
    float* side_item(int which) const { return side.get() + (size_t)n_cap * side_frame_floats(which); }   // TRS_TRAIN_SIDE_FIN .. DY3
    size_t side_array(int j) const { return j == 0 ? SL.w1y() : SL.off[kTrainArrays + j - 1]; }             // where side array j (0..6) lies in the four buffers
    float* item(int which) const { return fwd.get() + (size_t)n_cap * train_frame_floats(which); }   // TRS_TRAIN_DBG_OUT .. DELTA4
    float* dropped(int l) const                                                                      // a'(l), l = 1 .. 3
    {
        size_t o = 0;
        for (int j = 1; j < l; ++j) o += (size_t)kDropoutWidth[j];
        return drop.act.get() + (size_t)n_cap * o;
    }
};

// how every entry point behind trs_pilot_train_begin begins: the view, the pilot's tail and its open session
inline int enter_session(trs_env* e, TrsEnvView* v, TrsPilotTail* t, TrainSession** s)
{
    if (int rc = trs_internal_pilot_tail(e, v, t)) return rc;
    *s = static_cast<TrainSession*>(*t->train);
    if (!*s) return trs_internal_fail(TRS_ERR_STATE, "no training session on this pilot: trs_pilot_train_begin first");
    return TRS_OK;
}

// a binary16 value of a read-back as the float the debug entry points hand out
inline float widen_h(unsigned short u) { _Float16 h; std::memcpy(&h, &u, 2); return (float)h; }

// One backward pass and Adam over the trained convolutions, on the stream, from the tail's q1 [n padded to 64][128] and its exponent; before the tail's own
// Adam, with that step's constants.  x7_scale: dropout's s where the step dropped x7 (G7 takes it as one more factor), 0 where it did not: the plain
// kernel.  Defined in trsim_train_conv.hip, called by trs_pilot_train_step.
int trs_train_conv_step(ConvSession& s, trs_env* e, const TrsEnvView& v, const TrsPilotTail& t, const unsigned short* q1, const int* sexp1, int n,
                        const trsim_train_dev::AdamK& k, float x7_scale);

}  // namespace trsim
