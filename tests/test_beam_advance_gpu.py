"""msr3d_beam_advance and msr3d_greedy_advance (csrc/llm_beam.hip) against their statements (torch_beam_advance,
torch_greedy_advance, msr3d_amd/llm/search.py, run on the CPU), BIT FOR BIT on every field of the state after every step
of walks over made-up candidates -- no model.  The candidates are built to hold what can go wrong:
  exact ties across beams and inside a row (values are run_score + a multiple of -0.25, eight levels), and, made by
  hand at every step of every prompt, a tie across rank nb (the last candidate that may be kept as finished and the
  first that may not) and across rank K2 (the last candidate chosen and the first left out) -- at step 0 the latter is a
  tie between beam 0 and beam 1, the former one inside beam 0's row;
  an eos among the first nb candidates and among the rest (script "end": odd steps, prompt 0, ranks 0 and nb + 1);
  a step where every candidate is eos (script "all_eos": step 2, or the only step), which sets `done`;
  the last step, cur + 1 == L (script "end" runs into it);
  a prompt that stops (heur false) while its neighbours go on (script "heur": at step 1 all of prompt 0's first nb
  candidates end and its others are 100 lower, so its kept hypotheses are full and no running beam can beat them);
  a call after `done`, with other candidates: nothing may change.
Each walk asserts that its event happened, and each shape that the ties at both ranks, a tie between two beams, a tie
inside a row and an eos on either side of rank nb were in its candidates, so a change of the generator cannot empty a
case."""

import pytest
import torch

pytestmark = pytest.mark.gpu
EOS, PAD = 1, 0


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(gpu_state, cpu_state, what):
    for k, v in cpu_state.items():
        g = gpu_state[k].cpu()
        assert g.dtype == v.dtype and torch.equal(_bits(g), _bits(v)), (what, k, g, v)


def _kernel_beam(st, val, tok, d, out):
    from msr3d_amd._lib import call, current_stream_ptr, ptr
    B, nb, L = st["run_seq"].shape
    call("msr3d_beam_advance", B, nb, L, ptr(val), ptr(tok), EOS, ptr(d), ptr(st["run_scores"]), ptr(st["run_seq"]),
         ptr(st["fin_seq"]), ptr(st["fin_scores"]), ptr(st["fin_len"]), ptr(st["is_fin"].view(torch.uint8)),
         ptr(st["heur"].view(torch.uint8)), ptr(st["cur"]), ptr(st["done"]), ptr(out["next_tok"]), ptr(out["beam_idx"]),
         ptr(out["n_prev"]), ptr(out["work"]), current_stream_ptr())


def _candidates(g, st, script, step):
    """Made-up val, tok (B nb, 2 nb) for this step of `script` from the CPU state."""
    B, nb, L = st["run_seq"].shape
    K2 = 2 * nb
    q = -0.25 * torch.randint(0, 8, (B * nb, K2), generator=g).float()
    val = st["run_scores"].view(-1, 1) + q.sort(1, descending=True)[0]
    tok = torch.randint(2, 50, (B * nb, K2), generator=g, dtype=torch.int32)
    flat_t, flat_v = tok.view(B, nb * K2), val.view(B, nb * K2)
    ranks = lambda: torch.sort(flat_v, dim=1, descending=True, stable=True)[1]             # noqa: E731
    rows = torch.arange(B)
    for r in (nb, K2):                                       # rank r takes the value of rank r - 1 (the order stays sorted)
        order = ranks()
        flat_v[rows, order[:, r]] = flat_v[rows, order[:, r - 1]]
    order = ranks()                                          # (the ranks, to place an eos)
    if script == "all_eos" and (step == 2 or L <= 2):
        tok.fill_(EOS)
    elif script == "end" and step % 2 == 1:
        flat_t[0, order[0, 0]] = EOS
        flat_t[0, order[0, nb + 1]] = EOS
    elif script == "heur" and step == 1:
        flat_t[0, order[0, :nb]] = EOS
        rest = torch.ones(nb * K2, dtype=torch.bool)
        rest[order[0, :nb]] = False
        flat_v[0, rest] -= 100.0
    return val.contiguous(), tok.contiguous()


def _events(val, tok, nb):
    """What these candidates hold, by the statement's own order: a tie across rank nb, across rank K2, between two
    beams and inside one row among the first K2 + 1; an eos among the first nb and among the other chosen ones."""
    K2 = 2 * nb
    B = val.shape[0] // nb
    top, idx = torch.sort(val.view(B, nb * K2), dim=1, descending=True, stable=True)
    top, idx = top[:, :K2 + 1], idx[:, :K2 + 1]
    tied, same = top[:, 1:] == top[:, :-1], idx[:, 1:] // K2 == idx[:, :-1] // K2
    eos = torch.gather(tok.view(B, nb * K2), 1, idx[:, :K2]) == EOS
    return {"tie_at_nb": bool(tied[:, nb - 1].any()), "tie_at_K2": bool(tied[:, K2 - 1].any()),
            "tie_between_beams": bool((tied & ~same).any()), "tie_inside_a_row": bool((tied & same).any()),
            "eos_in_first_nb": bool(eos[:, :nb].any()), "eos_in_the_rest": bool(eos[:, nb:].any())}


@pytest.mark.parametrize("length_penalty", [0.5, 1.0, 2.0])
@pytest.mark.parametrize("L", [1, 7, 33])
@pytest.mark.parametrize("nb", [2, 5, 8, 32])
@pytest.mark.parametrize("B", [1, 3])
def test_beam_advance_equals_the_statement_bit_for_bit(B, nb, L, length_penalty):
    from msr3d_amd.llm.search import beam_state, length_divisors, torch_beam_advance
    seen = {}
    for script in ("end", "all_eos", "heur"):
        g = torch.Generator().manual_seed(1000 * B + 10 * nb + L)
        cpu, d = beam_state(B, nb, L, PAD), length_divisors(L, length_penalty)
        gpu, d_gpu = {k: v.cuda() for k, v in cpu.items()}, d.cuda()
        out = dict(next_tok=torch.zeros(B * nb, dtype=torch.int64, device="cuda"),
                   beam_idx=torch.zeros(B * nb, dtype=torch.int32, device="cuda"),
                   n_prev=torch.zeros(B * nb, dtype=torch.int32, device="cuda"),
                   work=torch.zeros(B, dtype=torch.int32, device="cuda"))
        seen_stop = False
        for step in range(L + 1):                            # (the last call comes after `done`)
            was_done = int(cpu["done"])
            val, tok = _candidates(g, cpu, script, step)
            if not was_done:
                for k, v in _events(val, tok, nb).items():
                    seen[k] = seen.get(k, False) or v
            cpu, next_tok, beam_idx = torch_beam_advance(cpu, val, tok, EOS, d)
            _kernel_beam(gpu, val.cuda(), tok.cuda(), d_gpu, out)
            what = (script, step)
            _same(gpu, cpu, what)
            if not was_done:
                assert torch.equal(out["next_tok"].cpu(), next_tok), what
                assert torch.equal(out["beam_idx"].cpu(), beam_idx), what
                assert bool((out["n_prev"].cpu() == step + 1).all()), what
                assert int(cpu["cur"]) == step + 1
                assert bool((cpu["run_seq"][:, :, step + 1:] == PAD).all())
                if script == "heur" and B > 1 and step >= 1 and not int(cpu["done"]):
                    seen_stop = seen_stop or cpu["heur"].tolist() == [False] + [True] * (B - 1)
            else:
                assert int(cpu["done"]) == 1                 # the call after `done` (compared field by field above)
        assert int(cpu["done"]) == 1
        if script == "end" and B > 1:
            assert int(cpu["cur"]) == L                      # ran into the last step
        if script == "all_eos":
            assert int(cpu["cur"]) == min(L, 3)
        if script == "heur" and B > 1 and L > 2:
            assert seen_stop
    assert all(seen.values()), seen


@pytest.mark.parametrize("N", [1, 64])
def test_greedy_advance_equals_the_statement(N):
    from msr3d_amd._lib import call, current_stream_ptr, ptr
    from msr3d_amd.llm.search import greedy_state, torch_greedy_advance
    for L, never in ((7, 9), (7, None), (1, 9)):             # rows n % never == 0 never emit eos; the others at step n % 5
        cpu = greedy_state(N, L, PAD)
        gpu = {k: v.cuda() for k, v in cpu.items()}
        next_tok = torch.zeros(N, dtype=torch.int64, device="cuda")
        n_prev = torch.zeros(N, dtype=torch.int32, device="cuda")
        g = torch.Generator().manual_seed(N + L)
        ends = []
        for step in range(L + 1):
            was_done = int(cpu["done"])
            tok = torch.randint(2, 50, (N, 1), generator=g, dtype=torch.int32)
            rows = torch.arange(N)
            ending = torch.ones(N, dtype=torch.bool) if never is None else rows % never != 0
            tok[ending & (rows % 5 == step), 0] = EOS
            cpu, nxt = torch_greedy_advance(cpu, tok, EOS, PAD)
            tg = tok.cuda()
            call("msr3d_greedy_advance", N, L, ptr(tg), 1, EOS, PAD, ptr(gpu["seq"]), ptr(gpu["unfinished"].view(torch.uint8)),
                 ptr(gpu["cur"]), ptr(gpu["done"]), ptr(next_tok), ptr(n_prev), current_stream_ptr())
            _same(gpu, cpu, (L, never, step))
            if not was_done:
                assert torch.equal(next_tok.cpu(), nxt) and bool((n_prev.cpu() == step + 1).all())
                ends.append(int(cpu["unfinished"].sum()))
        assert int(cpu["done"]) == 1
        if N == 64 and L == 7:
            assert len(set(ends)) > 2                        # rows finished at different steps
            assert int(cpu["cur"]) == (7 if never == 9 else 5)
