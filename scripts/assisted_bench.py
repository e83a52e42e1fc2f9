"""Cost of one round of assisted (speculative) greedy decoding on one MI355X: full size (GenVC_small dims: 30 layers,
d_model 1024, synthetic weights, fp32), ONE stream behind a 48-row prompt.

    python scripts/assisted_bench.py [--out profiles/assisted_decoding.md] [--json profiles/assisted_decoding.json] [--reps 5] [--render]

A round is k + 1 decode steps of the assistant (the pending token and the k drafts) plus one k + 1-row verification pass of the target,
the accept step and two rollbacks.  Its work does not depend on what is accepted, so one timing per (assistant layers, k) gives both
extremes: at acceptance 0 a round emits one token, at full acceptance k + 1.  Timed with device events around ONE engine call of
ROUNDS rounds that ends in a synchronise, after an untimed call of the same shape, REPS times per cell with the cells interleaved;
the cell's figure is the median and `spread` the largest relative distance of one timing from it.  The assistants are 2, 4 and 8 layer
models of the target's width with weights of their own (a truncated target is no valid draft, and is not what is timed here); with
synthetic weights they agree with the target about as often as chance, which is what makes every timed round emit exactly one token
-- the script asserts the count from the device counters -- and says NOTHING about the acceptance a trained draft model reaches.
The other extreme is run and reported, not timed: an assistant with the target's own weights (k + 1 tokens per round).
Next to the rounds, in the same process and interleaved with them: the plain one-stream greedy step of the same target
(engine.generate, 200 steps per call; DESIGN.md 4.1 has 513 us for it).
Break-even: a round must emit t_round / t_step tokens to match the plain loop.  With an independent per-draft acceptance probability
a, a round emits (1 - a^(k+1)) / (1 - a) tokens; the table gives the a at which that equals t_round / t_step ("never" when k + 1
tokens per round are not enough).

    python scripts/assisted_bench.py --sample [--sample_json profiles/assisted_sampling.json]

measures the round of speculative SAMPLING (GPT.generate(speculative_sampling=True), DESIGN.md 4.17: k full-sampler draft steps that
store their warped rows, one warp launch over the k + 1 verification rows, the accept kernel) at top_k = 15, top_p = 0.85, temperature
0.85 on the same cells, interleaved in one process with the greedy round of the same cell and with the plain SAMPLED step of the
target at the same settings, and adds its section to --out behind the greedy report (rendered from --json as it stands).

    python scripts/assisted_bench.py --lookup [--lookup_json profiles/assisted_lookup.json]

measures the round of PROMPT-LOOKUP decoding (GPT.generate(prompt_lookup_num_tokens=k), DESIGN.md 4.18: one lookup launch, the
(k + 1)-row verification pass, accept, one rollback; no assistant) at max_matching_ngram_size = 2 for k = 3 / 5 / 7, greedy and
sampled (the settings of --sample), twice per cell: as the call runs on this model (the drafted and accepted counts are reported), and
with the lookup's `from` moved behind the ids row so that no round finds a match (every round emits exactly one token, asserted) --
the price every stream pays whatever it drafts.  Interleaved in one process with the plain greedy and sampled steps; its section
follows the others in --out."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LAYERS = (2, 4, 8)
KS = (3, 5, 7)
NGRAM = 2          # max_matching_ngram_size of the lookup cells (GPT.generate's default)
ROUNDS = 40
STEPS = 200
MAX_NEW = 400


def med(xs):
    return sorted(xs)[len(xs) // 2]


def build(layers, seed, weights=None):
    from genvc_amd import config as gcfg
    from genvc_amd import synth
    from genvc_amd.layers.gpt import GPT
    a = dict(gcfg.DEFAULT_MODEL_ARGS, gpt_layers=layers)
    g = GPT(layers=a["gpt_layers"], model_dim=a["gpt_n_model_channels"], heads=a["gpt_n_heads"],
            max_text_tokens=a["gpt_max_text_tokens"], max_mel_tokens=a["gpt_max_audio_tokens"],
            max_prompt_tokens=a["gpt_max_prompt_tokens"], number_text_tokens=a["gpt_number_text_tokens"],
            start_text_token=a["gpt_start_text_token"], stop_text_token=a["gpt_stop_text_token"],
            num_audio_tokens=a["gpt_num_audio_tokens"], start_audio_token=a["gpt_start_audio_token"],
            stop_audio_token=a["gpt_stop_audio_token"], code_stride_len=a["gpt_code_stride_len"])
    if weights is None:
        weights = synth.make_weights(seed, synth.gpt_weight_spec(gcfg.gpt_dims(a)))
        weights["mel_head.bias"][1025] = -30.0          # the stop token is biased away: every run takes all its rounds
    g.load_state_dict(weights, strict=False)
    g.to("cuda")
    g.init_gpt_for_inference(max_slots=2)
    return g, weights


def break_even(tokens_needed, k):
    """the per-draft acceptance probability a with (1 - a^(k+1)) / (1 - a) = tokens_needed, None when k + 1 tokens are not enough"""
    if tokens_needed <= 1.0:
        return 0.0
    if tokens_needed >= k + 1:
        return None
    lo, hi = 0.0, 1.0
    for _ in range(60):
        a = 0.5 * (lo + hi)
        e = sum(a ** i for i in range(k + 1))
        lo, hi = (a, hi) if e < tokens_needed else (lo, a)
    return 0.5 * (lo + hi)


def measure(args):
    import torch
    from genvc_amd import synth
    from genvc_amd.engine import AssistedState, sample_params
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    target, w30 = build(30, 1)
    twin, _ = build(30, 1, weights=w30)
    assistants = {n: build(n, 7)[0] for n in LAYERS}
    d = target.model_dim
    cond = synth.uniform(300, "cond_latents", (1, 32, d), 1.0).cuda()
    codes = synth.integers(300, "content_codes", (1, 13), 256).cuda()
    fake = target.compute_embeddings(cond, codes)
    for g in [twin] + list(assistants.values()):
        g.compute_embeddings(cond, codes)
    n0 = int(fake.shape[1])
    assert n0 == 48
    slots = torch.zeros(1, device="cuda", dtype=torch.int32)
    params = sample_params(dict(repetition_penalty=1.0, temperature=1.0, top_p=1.0, top_k=1), 1026, 1025)
    teng = target.engine

    def rounds(asst, k, n_rounds):
        """prefill both (untimed), then the opening step and n_rounds rounds in one timed call -> (us per round, state)"""
        teng.prefill(slots, target._prefix, want_outputs=False)
        asst.engine.prefill(slots, asst._prefix, want_outputs=False)
        st = AssistedState(fake, k, MAX_NEW, 1025, 1026, d)
        reach = 1 + n_rounds * (k + 1) + k
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        teng.generate_assisted(asst.engine, slots, slots, st, params, n_rounds, n0 + reach, n0 + reach)
        e1.record()
        torch.cuda.synchronize()
        teng.health()
        asst.engine.health()
        return e0.elapsed_time(e1) * 1000.0 / n_rounds, st

    def plain():
        teng.prefill(slots, target._prefix, want_outputs=False)
        ids = torch.ones(1, n0 + STEPS + 8, device="cuda", dtype=torch.int32)
        ids[:, n0 - 1] = 1024
        ids_len = torch.full((1,), n0, device="cuda", dtype=torch.int32)
        fin = torch.zeros(1, device="cuda", dtype=torch.int32)
        toks = torch.zeros(1, STEPS, device="cuda", dtype=torch.int32)
        lats = torch.zeros(1, STEPS, d, device="cuda")
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        teng.generate(slots, ids, ids_len, fin, params, 0, STEPS, toks, lats, max_keys=n0 + STEPS)
        e1.record()
        torch.cuda.synchronize()
        teng.health()
        return e0.elapsed_time(e1) * 1000.0 / STEPS, toks

    # the other extreme, checked and reported (not timed): the target's own weights as the assistant
    plain_toks = plain()[1][0, :40].tolist()
    plain_variant = teng.decode_variant()
    twin_rows = []
    for k in KS:
        _, st = rounds(twin, k, 3)
        s = st.stats()
        n = int(st.emitted[0])
        twin_rows.append(dict(k=k, rounds=3, drafted=int(s["drafted"][0]), accepted=int(s["accepted"][0]), emitted=n,
                              tokens_equal_plain=st.toks[0, :n].tolist() == plain_toks[:n]))
    cells = {(n, k): [] for n in LAYERS for k in KS}
    steps = []
    for n, k in cells:          # untimed: every shape once
        rounds(assistants[n], k, ROUNDS)
    plain()
    accepted = {}
    for _ in range(args.reps):
        steps.append(plain()[0])
        for (n, k), xs in cells.items():
            us, st = rounds(assistants[n], k, ROUNDS)
            xs.append(us)
            accepted[(n, k)] = int(st.stats()["accepted"][0])
            assert int(st.emitted[0]) == 1 + ROUNDS + accepted[(n, k)] and int(st.stats()["rounds"][0]) == ROUNDS
    t_step = med(steps)
    res = dict(device=torch.cuda.get_device_name(0), n0=n0, rounds_per_call=ROUNDS, steps_per_plain_call=STEPS, reps=args.reps,
               plain_us_per_step=t_step, plain_runs=steps, plain_spread=max(abs(x - t_step) / t_step for x in steps),
               plain_variant=plain_variant, own_weights_assistant=twin_rows, cells=[])
    for (n, k), xs in cells.items():
        t = med(xs)
        res["cells"].append(dict(assistant_layers=n, k=k, us_per_round=t, spread=max(abs(x - t) / t for x in xs), runs=xs,
                                 us_per_token_acceptance_0=t, us_per_token_full_acceptance=t / (k + 1),
                                 tokens_per_round_to_break_even=t / t_step, break_even_acceptance=break_even(t / t_step, k),
                                 accepted_in_last_timed_call=accepted[(n, k)]))
    return res


SAMPLING = dict(repetition_penalty=1.0, temperature=0.85, top_p=0.85, top_k=15)


def measure_sample(args):
    """the sampled round against the greedy round of the same cell and the plain sampled step, one process, interleaved"""
    import torch
    from genvc_amd import synth
    from genvc_amd.engine import AssistedState, sample_params
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    target, _ = build(30, 1)
    assistants = {n: build(n, 7)[0] for n in LAYERS}
    d = target.model_dim
    cond = synth.uniform(300, "cond_latents", (1, 32, d), 1.0).cuda()
    codes = synth.integers(300, "content_codes", (1, 13), 256).cuda()
    fake = target.compute_embeddings(cond, codes)
    for g in assistants.values():
        g.compute_embeddings(cond, codes)
    n0 = int(fake.shape[1])
    slots = torch.zeros(1, device="cuda", dtype=torch.int32)
    greedy = sample_params(dict(repetition_penalty=1.0, temperature=1.0, top_p=1.0, top_k=1), 1026, 1025)
    sampled = sample_params(SAMPLING, 1026, 1025, 17)
    teng = target.engine

    def rounds(asst, k, sample):
        teng.prefill(slots, target._prefix, want_outputs=False)
        asst.engine.prefill(slots, asst._prefix, want_outputs=False)
        st = AssistedState(fake, k, MAX_NEW, 1025, 1026, d)
        reach = 1 + ROUNDS * (k + 1) + k
        more = dict(sampling=True) if sample else {}
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        teng.generate_assisted(asst.engine, slots, slots, st, sampled if sample else greedy, ROUNDS, n0 + reach, n0 + reach, **more)
        e1.record()
        torch.cuda.synchronize()
        teng.health()
        asst.engine.health()
        s = st.stats()
        assert int(s["rounds"][0]) == ROUNDS and int(st.emitted[0]) == 1 + ROUNDS + int(s["accepted"][0])
        return e0.elapsed_time(e1) * 1000.0 / ROUNDS, int(s["accepted"][0]), int(s["drafted"][0])

    def plain(params):
        teng.prefill(slots, target._prefix, want_outputs=False)
        ids = torch.ones(1, n0 + STEPS + 8, device="cuda", dtype=torch.int32)
        ids[:, n0 - 1] = 1024
        ids_len = torch.full((1,), n0, device="cuda", dtype=torch.int32)
        fin = torch.zeros(1, device="cuda", dtype=torch.int32)
        toks = torch.zeros(1, STEPS, device="cuda", dtype=torch.int32)
        lats = torch.zeros(1, STEPS, d, device="cuda")
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        teng.generate(slots, ids, ids_len, fin, params, 0, STEPS, toks, lats, max_keys=n0 + STEPS)
        e1.record()
        torch.cuda.synchronize()
        teng.health()
        return e0.elapsed_time(e1) * 1000.0 / STEPS

    cells = {(n, k): dict(sampled=[], greedy=[]) for n in LAYERS for k in KS}
    for n, k in cells:          # untimed: every shape once in both modes
        rounds(assistants[n], k, True)
        rounds(assistants[n], k, False)
    plain(sampled)
    plain(greedy)
    steps, gsteps, acc = [], [], {}
    for _ in range(args.reps):
        steps.append(plain(sampled))
        gsteps.append(plain(greedy))
        for (n, k), xs in cells.items():
            us, a, dr = rounds(assistants[n], k, True)
            xs["sampled"].append(us)
            acc[(n, k)] = (a, dr)
            xs["greedy"].append(rounds(assistants[n], k, False)[0])
    t_step, g_step = med(steps), med(gsteps)
    res = dict(device=torch.cuda.get_device_name(0), n0=n0, rounds_per_call=ROUNDS, steps_per_plain_call=STEPS, reps=args.reps,
               sampling=SAMPLING, plain_sampled_us_per_step=t_step, plain_sampled_runs=steps,
               plain_sampled_spread=max(abs(x - t_step) / t_step for x in steps), plain_greedy_us_per_step=g_step,
               plain_greedy_runs=gsteps, cells=[])
    for (n, k), xs in cells.items():
        ts, tg = med(xs["sampled"]), med(xs["greedy"])
        res["cells"].append(dict(assistant_layers=n, k=k, sampled_us_per_round=ts, greedy_us_per_round=tg,
                                 sampled_spread=max(abs(x - ts) / ts for x in xs["sampled"]),
                                 greedy_spread=max(abs(x - tg) / tg for x in xs["greedy"]), sampled_runs=xs["sampled"],
                                 greedy_runs=xs["greedy"], tokens_per_round_to_break_even=ts / t_step,
                                 break_even_acceptance=break_even(ts / t_step, k), accepted_in_last_timed_call=acc[(n, k)][0],
                                 drafted_in_last_timed_call=acc[(n, k)][1]))
    return res


def render_sample(res):
    """the section on speculative sampling (every figure in it is computed from `res`)"""
    t_step, s = res["plain_sampled_us_per_step"], res["sampling"]
    lines = ["", "## Speculative sampling: the cost of a sampled round", "",
             f"`scripts/assisted_bench.py --sample` on one MI355X ({res['device']}): the same target, assistants, prompt and cells; "
             f"top_k = {s['top_k']}, top_p = {s['top_p']}, temperature = {s['temperature']}; {res['rounds_per_call']} rounds per timed call, "
             f"{res['reps']} timed calls per cell and mode (median; spread as above), the sampled round, the greedy round of the same "
             "cell and the plain loops interleaved in one process.  Timed with device events around one engine call that ends in a "
             "synchronise, after an untimed call of every shape.", "",
             f"Plain one-stream SAMPLED step of the same target at these settings, same run: **{t_step:.1f} us** per token over "
             f"{res['steps_per_plain_call']} steps (spread {res['plain_sampled_spread']:.2%}); the plain greedy step in this run: "
             f"{res['plain_greedy_us_per_step']:.1f} us.", "",
             "A sampled round = a greedy round with k full-sampler draft steps that also store their warped row (instead of k argmax "
             "steps), one warp launch of k + 1 workgroups and the accept kernel (instead of the greedy accept kernel).  Break-even is "
             "against the plain SAMPLED step.", "",
             "| assistant layers | k | sampled us / round | spread | greedy us / round | spread | sampled - greedy | tokens / round to break "
             "even | break-even per-draft acceptance |", "|---|---|---|---|---|---|---|---|---|"]
    for c in res["cells"]:
        ts, tg, a = c["sampled_us_per_round"], c["greedy_us_per_round"], c["break_even_acceptance"]
        lines.append(f"| {c['assistant_layers']} | {c['k']} | {ts:.0f} | {c['sampled_spread']:.2%} | {tg:.0f} | {c['greedy_spread']:.2%} | "
                     f"{ts - tg:+.0f} | {ts / t_step:.2f} | {'never' if a is None else f'{a:.2f}'} |")
    acc = ", ".join(f"{c['accepted_in_last_timed_call']} of {c['drafted_in_last_timed_call']}" for c in res["cells"])
    lines += ["", "The acceptance of a sampled round is min(1, p / q) per draft, not agreement of two argmaxes; with synthetic weights the "
              f"unrelated assistants had {acc} drafts accepted in the last timed call of each cell, which says nothing about a trained "
              "draft model.  What was measured is the cost of a round; no threshold was set for it in advance."]
    return "\n".join(lines) + "\n"


def measure_lookup(args):
    """the lookup round, greedy and sampled, natural and without any match, against the plain steps: one process, interleaved"""
    import torch
    from genvc_amd import synth
    from genvc_amd.engine import AssistedState, sample_params
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    target, _ = build(30, 1)
    d = target.model_dim
    cond = synth.uniform(300, "cond_latents", (1, 32, d), 1.0).cuda()
    codes = synth.integers(300, "content_codes", (1, 13), 256).cuda()
    fake = target.compute_embeddings(cond, codes)
    n0 = int(fake.shape[1])
    slots = torch.zeros(1, device="cuda", dtype=torch.int32)
    greedy = sample_params(dict(repetition_penalty=1.0, temperature=1.0, top_p=1.0, top_k=1), 1026, 1025)
    sampled = sample_params(SAMPLING, 1026, 1025, 17)
    teng = target.engine

    def rounds(k, sample, match):
        teng.prefill(slots, target._prefix, want_outputs=False)
        st = AssistedState(fake, k, MAX_NEW, 1025, 1026, d)
        if not match:
            st.n0 = int(st.ids.shape[1])          # the lookup's `from` behind the ids row: an empty history, draft_len 0 in every round
        reach = 1 + ROUNDS * (k + 1) + k
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        teng.generate_lookup(slots, st, sampled if sample else greedy, ROUNDS, n0 + reach, NGRAM, k=k, sampling=sample)
        e1.record()
        torch.cuda.synchronize()
        teng.health()
        s = st.stats()
        assert int(s["rounds"][0]) == ROUNDS and int(st.emitted[0]) == 1 + ROUNDS + int(s["accepted"][0])
        assert match or (int(s["drafted"][0]) == 0 and int(st.emitted[0]) == 1 + ROUNDS)
        return e0.elapsed_time(e1) * 1000.0 / ROUNDS, int(s["accepted"][0]), int(s["drafted"][0]), int(st.emitted[0])

    def plain(params):
        teng.prefill(slots, target._prefix, want_outputs=False)
        ids = torch.ones(1, n0 + STEPS + 8, device="cuda", dtype=torch.int32)
        ids[:, n0 - 1] = 1024
        ids_len = torch.full((1,), n0, device="cuda", dtype=torch.int32)
        fin = torch.zeros(1, device="cuda", dtype=torch.int32)
        toks = torch.zeros(1, STEPS, device="cuda", dtype=torch.int32)
        lats = torch.zeros(1, STEPS, d, device="cuda")
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        teng.generate(slots, ids, ids_len, fin, params, 0, STEPS, toks, lats, max_keys=n0 + STEPS)
        e1.record()
        torch.cuda.synchronize()
        teng.health()
        return e0.elapsed_time(e1) * 1000.0 / STEPS

    cells = {(k, sample, match): [] for k in KS for sample in (False, True) for match in (True, False)}
    for c in cells:          # untimed: every shape once
        rounds(*c)
    plain(greedy)
    plain(sampled)
    gsteps, ssteps, seen = [], [], {}
    for _ in range(args.reps):
        gsteps.append(plain(greedy))
        ssteps.append(plain(sampled))
        for c, xs in cells.items():
            us, acc, dr, em = rounds(*c)
            xs.append(us)
            seen[c] = (acc, dr, em)
    g_step, s_step = med(gsteps), med(ssteps)
    res = dict(device=torch.cuda.get_device_name(0), n0=n0, rounds_per_call=ROUNDS, steps_per_plain_call=STEPS, reps=args.reps,
               max_matching_ngram_size=NGRAM, sampling=SAMPLING, plain_greedy_us_per_step=g_step, plain_greedy_runs=gsteps,
               plain_greedy_spread=max(abs(x - g_step) / g_step for x in gsteps), plain_sampled_us_per_step=s_step,
               plain_sampled_runs=ssteps, plain_sampled_spread=max(abs(x - s_step) / s_step for x in ssteps), cells=[])
    for (k, sample, match), xs in cells.items():
        t, step = med(xs), s_step if sample else g_step
        res["cells"].append(dict(k=k, sampled=sample, lookups_match=match, us_per_round=t, spread=max(abs(x - t) / t for x in xs), runs=xs,
                                 plain_us_per_step=step, tokens_per_round_to_break_even=t / step,
                                 accepted_in_last_timed_call=seen[(k, sample, match)][0],
                                 drafted_in_last_timed_call=seen[(k, sample, match)][1],
                                 emitted_in_last_timed_call=seen[(k, sample, match)][2]))
    return res


def render_lookup(res):
    """the section on prompt-lookup decoding (every figure in it is computed from `res`)"""
    g, s = res["plain_greedy_us_per_step"], res["plain_sampled_us_per_step"]
    sm = res["sampling"]
    lines = ["", "## Prompt lookup: the cost of a round without a draft model", "",
             f"`scripts/assisted_bench.py --lookup` on one MI355X ({res['device']}): the same target and prompt, no assistant; "
             f"max_matching_ngram_size = {res['max_matching_ngram_size']}; sampled cells at top_k = {sm['top_k']}, top_p = {sm['top_p']}, "
             f"temperature = {sm['temperature']}; {res['rounds_per_call']} rounds per timed call, {res['reps']} timed calls per cell (median; "
             "spread as above), all cells and the plain loops interleaved in one process.  Timed with device events around one engine "
             "call that ends in a synchronise, after an untimed call of every shape.", "",
             f"Plain one-stream steps of the same target, same run: greedy **{g:.1f} us** per token (spread "
             f"{res['plain_greedy_spread']:.2%}), sampled **{s:.1f} us** (spread {res['plain_sampled_spread']:.2%}), over "
             f"{res['steps_per_plain_call']} steps each.", "",
             "A lookup round = one lookup launch + one (k + 1)-row verification pass + accept (sampled: put-drafts, warp and accept "
             "launches) + one rollback, launched directly (no graph).  \"no match\" rows: the same call with the lookup's `from` moved "
             "behind the ids row, so every round has draft_len = 0 and emits exactly one token (asserted) -- the verification pass "
             "still runs all k + 1 rows.  Tokens / round to break even = (us / round) / (plain us / token of the same mode).", "",
             "| mode | k | lookups | us / round | spread | plain us / token | round - plain step | tokens / round to break even | drafted | "
             "accepted | tokens emitted |", "|---|---|---|---|---|---|---|---|---|---|---|"]
    for c in res["cells"]:
        t, p = c["us_per_round"], c["plain_us_per_step"]
        lines.append(f"| {'sampled' if c['sampled'] else 'greedy'} | {c['k']} | {'as they fall' if c['lookups_match'] else 'no match'} | "
                     f"{t:.0f} | {c['spread']:.2%} | {p:.1f} | {t - p:+.0f} ({(t - p) / p:+.1%}) | {t / p:.2f} | "
                     f"{c['drafted_in_last_timed_call']} | {c['accepted_in_last_timed_call']} | {c['emitted_in_last_timed_call']} |")
    nm = [c for c in res["cells"] if not c["lookups_match"]]
    worse = [c for c in nm if c["us_per_round"] > c["plain_us_per_step"]]
    lines += ["", ("A round without any match costs MORE than a plain step in " + ("every" if len(worse) == len(nm) else f"{len(worse)} of "
               f"{len(nm)}") + " measured cells: " if worse else "A round without any match costs no more than a plain step: ") +
              "; ".join(f"{'sampled' if c['sampled'] else 'greedy'} k = {c['k']}: {c['us_per_round'] - c['plain_us_per_step']:+.0f} us "
                        f"({(c['us_per_round'] - c['plain_us_per_step']) / c['plain_us_per_step']:+.1%})" for c in nm) +
              ".  That is what a stream that never repeats itself pays per token for the mode; a stream gains as soon as its rounds emit "
              "more tokens on average than the break-even column says.", "",
              "The drafted / accepted / emitted columns of the \"as they fall\" rows are what this SYNTHETIC model did in the last timed "
              f"call ({res['rounds_per_call']} rounds): they show the mode at work and say nothing about a trained checkpoint, whose code "
              "streams repeat where speech pauses or sustains, not where random weights happen to loop.  No threshold was set for these "
              "figures in advance."]
    return "\n".join(lines) + "\n"


LOOKUP_PENDING = ("\n## Prompt lookup: the cost of a round without a draft model\n\nNot measured yet: `scripts/assisted_bench.py --lookup` has not "
                  "run on a GPU, so no figure is given here.  It times the lookup round (one lookup launch, the (k + 1)-row verification pass, "
                  "accept, one rollback; max_matching_ngram_size = 2) at k = 3 / 5 / 7, greedy and sampled, as the call runs on the synthetic "
                  "model and with every lookup forced to find no match, beside the plain greedy and sampled steps in the same process; it "
                  "writes `profiles/assisted_lookup.json` and replaces this section with the table, the tokens per round that break even, "
                  "the drafted and accepted counts on the synthetic model, and by how much a round without any match exceeds a plain "
                  "step.\n")

RATES = (0.5, 0.6, 0.7, 0.8, 0.9)


def render(res):
    """the markdown report of a measurement (every figure in it is computed from `res`)"""
    t_step = res["plain_us_per_step"]
    lines = ["# Assisted (speculative) greedy decoding: the cost of a round", "",
             f"`scripts/assisted_bench.py` on one MI355X (device name as the runtime reports it: {res['device']}): 30 layers, d_model 1024, "
             f"fp32, one stream, a {res['n0']}-row prompt; {res['rounds_per_call']} rounds per timed call, {res['reps']} timed calls per "
             "cell (median; `spread` is the largest relative distance of one call from it), cells interleaved with the plain loop in one "
             "process.", "",
             f"Plain one-stream greedy step of the same target, same run: **{t_step:.1f} us** per token over "
             f"{res['steps_per_plain_call']} steps, sampler included (spread {res['plain_spread']:.2%}; DESIGN.md 4.1 has 513 us for the "
             "decode step alone at the headline workload's context lengths).", "",
             "A round = k + 1 assistant decode steps + one (k + 1)-row verification pass + accept + two rollbacks, launched directly "
             "(no graph).  Its work is the same whatever is accepted: at acceptance 0 it emits 1 token, at full acceptance k + 1.", "",
             "| assistant layers | k | us / round | spread | us / token, acceptance 0 | us / token, full acceptance | tokens / round to "
             "break even | break-even per-draft acceptance |", "|---|---|---|---|---|---|---|---|"]
    for c in res["cells"]:
        t, k, a = c["us_per_round"], c["k"], c["break_even_acceptance"]
        lines.append(f"| {c['assistant_layers']} | {k} | {t:.0f} | {c['spread']:.2%} | {t:.0f} | {t / (k + 1):.0f} | {t / t_step:.2f} | "
                     f"{'never' if a is None else f'{a:.2f}'} |")
    lines += ["", "Break-even: a round has to emit (us / round) / (plain us / token) tokens; the last column is the independent per-draft "
              "acceptance probability a at which (1 - a^(k+1)) / (1 - a) reaches that.", "",
              "Expected us per token, (us / round) / ((1 - a^(k+1)) / (1 - a)), at a per-draft acceptance a (computed from the table above; "
              f"the plain loop is {t_step:.0f}):", "", "| assistant layers | k | " + " | ".join(f"a = {a}" for a in RATES) + " |",
              "|---|---|" + "---|" * len(RATES)]
    for c in res["cells"]:
        k = c["k"]
        lines.append(f"| {c['assistant_layers']} | {k} | " +
                     " | ".join(f"{c['us_per_round'] / sum(a ** i for i in range(k + 1)):.0f}" for a in RATES) + " |")
    acc = sorted({c["accepted_in_last_timed_call"] for c in res["cells"]})
    # the default k: the one whose expected cost is never far from the best of the measured three, over every (size, a) at which
    # assisted decoding beats the plain loop at all
    exp = {(c["assistant_layers"], c["k"], a): c["us_per_round"] / sum(a ** i for i in range(c["k"] + 1)) for c in res["cells"] for a in RATES}
    sizes, ks = sorted({c["assistant_layers"] for c in res["cells"]}), sorted({c["k"] for c in res["cells"]})
    regret = {k: 0.0 for k in ks}
    for n in sizes:
        for a in RATES:
            best = min(exp[(n, k, a)] for k in ks)
            if best < t_step:
                for k in ks:
                    regret[k] = max(regret[k], exp[(n, k, a)] / best - 1.0)
    pick = min(ks, key=lambda k: regret[k])
    lines += ["", "Reading for the default `num_assistant_tokens`: over every (assistant size, a) above at which some k beats the plain "
              "loop, the worst excess of a k over the best of the three is " + ", ".join(f"k = {k}: +{regret[k]:.0%}" for k in ks) +
              f".  k = {pick} is never far from the best; small k wins at low acceptance, large k at high.  GPT.generate's default is 5.",
              "", "The weights are synthetic.  The unrelated assistants agree with the target about as often as chance (the timed calls "
              f"accepted {acc} drafts in {res['rounds_per_call']} rounds), and an assistant with the target's own weights gave " +
              "; ".join(f"k = {r['k']}: {r['accepted']} of {r['drafted']} drafts accepted, {r['emitted']} tokens in {r['rounds']} rounds, "
                        f"tokens {'equal to' if r['tokens_equal_plain'] else 'DIFFERENT from'} the plain loop's"
                        for r in res["own_weights_assistant"]) +
              ".  These pin the two ends of the range and say nothing about the acceptance rate a trained draft model would reach."]
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "assisted_decoding.md"))
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "assisted_decoding.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--render", action="store_true", help="no measurement: write --out again from the figures in --json")
    ap.add_argument("--sample", action="store_true", help="measure the round of speculative sampling (into --sample_json); the greedy "
                                                          "report is rendered from --json as it stands")
    ap.add_argument("--sample_json", default=os.path.join(ROOT, "profiles", "assisted_sampling.json"))
    ap.add_argument("--lookup", action="store_true", help="measure the round of prompt-lookup decoding (into --lookup_json); the other "
                                                          "reports are rendered from their json files as they stand")
    ap.add_argument("--lookup_json", default=os.path.join(ROOT, "profiles", "assisted_lookup.json"))
    args = ap.parse_args()
    if args.lookup:
        lres = measure_lookup(args)
        with open(args.lookup_json, "w") as f:
            json.dump(lres, f, indent=1)
    if args.sample:
        sres = measure_sample(args)
        with open(args.sample_json, "w") as f:
            json.dump(sres, f, indent=1)
    if args.render or args.sample or args.lookup:
        with open(args.json) as f:
            res = json.load(f)
    else:
        res = measure(args)
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
    text = render(res)
    if os.path.exists(args.sample_json):
        with open(args.sample_json) as f:
            text += render_sample(json.load(f))
    if os.path.exists(args.lookup_json):
        with open(args.lookup_json) as f:
            text += render_lookup(json.load(f))
    else:
        text += LOOKUP_PENDING
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
