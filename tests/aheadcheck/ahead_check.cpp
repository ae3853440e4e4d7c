// Host check of trc_stream_form_ahead (tracer_amd/csrc/trc_forms.h): whether k_s_shade_c finishes the next segment of the continued
// rays inside their clear cones.  The fact blocks are hostcheck.cpp's (hc_facts_of, included here with its entry points), which know
// nothing of what the decision reads beyond them; those three facts come beside every block.
#include "../hostcheck/hostcheck.cpp"

extern "C" {

// n fact blocks of HC_FACTS doubles, and per block more[3] = the scene has clear cones, TRC_STREAM_CLEAR, TRC_STREAM_AHEAD (as the knobs
// end up: 1 unless set to 0).  out, per block: the streaming forms were decided, the path is on.  With more == null the three are what
// a fact block that does not name them gets: no cones, both knobs at their defaults.
int ac_ahead(long n, const double *facts, const double *more, double *out) {
    for (long i = 0; i < n; ++i) {
        trc_facts f = hc_facts_of(facts + (size_t)HC_FACTS * i);
        if (more) {
            f.scene.clear_cones = more[3 * i] != 0.0;
            f.knobs.clear = more[3 * i + 1] != 0.0;
            f.knobs.ahead = more[3 * i + 2] != 0.0;
        }
        StreamPlan plan = {0, 0, true};
        const bool ok = stream_plan(f.scene, (f.call.flags & TRC_TRACE_ACCEL) != 0, f.knobs, &plan);
        trc_stream_forms F;
        f.call.carry = f.call.carry || f.scene.splits;
        const bool decided = ok && trc_stream_decide(f, plan, &F);
        out[2 * i] = decided;
        out[2 * i + 1] = decided && F.ahead;
    }
    return 2;
}

}  // extern "C"
