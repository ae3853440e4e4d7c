"""
GPU tests of the search kernel instances of the streaming engine (k_s_cull, k_s_fresh, k_s_fresh2, k_s_bounce, k_s_bounce_coop, k_s_walk,
k_s_gen, k_s_gen_src, k_s_exact: 79 compiled kernels, picked per call by stream_plan and the trc_stream_form_* functions), run with -m gpu
on the MI355X box.

Every call of search_cases.py -- a scene, a source or its rays given, accel, a Kd-tree, knobs, a first or a second call;
test_search_cases_host.py checks the selection and the conditions on the inputs without a device -- is traced by the streaming form
and held to oracle.engine on the same Philox streams by the assertions of test_gpu_shade_instances._check: hit counts per surface
exactly, the call's statistics, every surviving ray, every captured hit (two lean captures and a full one), and the flux map against
numpy.histogram2d of the oracle's hits.  No ray is excluded.  Every scene holds a twin -- two plates of one frame and one size -- whose
hits the reference gives to the lower index: a search that breaks the tie the other way, or loses a candidate, shows in the hit
counts.  The megakernel is held to the same assertions once per scene and rays.  Which instances these calls launched is recorded in
profiles/search_instances.txt from a kernel trace of this file.
"""
import pytest

import search_cases as S
from test_gpu_shade_instances import _check, ctx        # noqa: F401 (ctx: the module's fixture)

pytestmark = pytest.mark.gpu


def _ids(name):
    return '%s[%s]' % (name, '+'.join(t.replace(' ', '') for t in S.CALL[name].targets))


@pytest.mark.parametrize('name', [c.name for c in S.CALLS], ids=_ids)
def test_streaming_call_against_the_oracle(ctx, name):
    c = S.CALL[name]
    _check(ctx, c, S.reference(c), c.given, True, (name, 'stream'), accel=c.accel, kd=S.scene(c.scene).kdtree() if c.kd else None,
           scene_knobs=dict(c.scene_env), warm_up=c.second, **dict(c.env))


# one call per (scene, rays): the first of CALLS that traces them
FIRST_OF = {}
for _c in S.CALLS:
    FIRST_OF.setdefault((_c.scene, _c.src), _c.name)


@pytest.mark.parametrize('name', sorted(FIRST_OF.values()))
def test_megakernel_against_the_oracle(ctx, name):
    """the same scene and source with stream=False: places a failure in the streaming path or in the shared per-ray core"""
    c = S.CALL[name]
    _check(ctx, c, S.reference(c), False, False, (name, 'megakernel'))
