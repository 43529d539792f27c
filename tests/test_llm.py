"""LLM stack tests: LoRA, fused logprobs, GRPO/SFT/DPO on a tiny random Llama."""

import os

import numpy as np
import pytest
import torch

from agilerl_amd import ops
from agilerl_amd.llm import (
    LoraConfig,
    adapter_state_dict,
    add_adapter,
    apply_lora,
    load_adapter_state_dict,
    set_active_adapter,
)
from agilerl_amd.ops.fused_logprobs import fused_linear_logprobs
from agilerl_amd.ops.grpo_loss import grpo_policy_loss

# the reference project's training YAMLs, stored verbatim
REF_CONFIGS = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                           "golden", "reference_configs", "training")

TINY = dict(
    model_type="llama", vocab_size=128, hidden_size=64, intermediate_size=128,
    num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
    max_position_embeddings=256, pad_token_id=0,
)


def tiny_agent(cls, **kw):
    kw.setdefault("dtype", torch.float32)
    kw.setdefault("lora_config", {"r": 4, "lora_alpha": 8})
    kw.setdefault("micro_batch_size", 4)
    return cls(model_config=dict(TINY), **kw)


class TestLora:
    def _model(self):
        import torch.nn as nn

        class M(nn.Module):
            def __init__(self):
                super().__init__()
                self.q_proj = nn.Linear(16, 16)
                self.other = nn.Linear(16, 16)

            def forward(self, x):
                return self.q_proj(x) + self.other(x)

        return M()

    def test_wrap_and_zero_delta(self):
        m = self._model()
        x = torch.randn(3, 16)
        y0 = m(x)
        apply_lora(m, LoraConfig(r=4, target_modules=["q_proj"]), adapters=["actor"])
        y1 = m(x)
        torch.testing.assert_close(y0, y1)  # B=0 init -> identity delta

    def test_adapter_isolation(self):
        m = self._model()
        apply_lora(m, LoraConfig(r=4, target_modules=["q_proj"]), adapters=["a", "b"])
        x = torch.randn(3, 16)
        with torch.no_grad():
            m.q_proj.lora_B["a"].fill_(1.0)
        set_active_adapter(m, "a")
        ya = m(x)
        set_active_adapter(m, "b")
        yb = m(x)
        set_active_adapter(m, None)
        yn = m(x)
        assert not torch.allclose(ya, yb)
        torch.testing.assert_close(yb, yn)  # b still zero-delta

    def test_state_roundtrip(self):
        m = self._model()
        apply_lora(m, LoraConfig(r=4, target_modules=["q_proj"]), adapters=["a"])
        with torch.no_grad():
            m.q_proj.lora_A["a"].normal_()
            m.q_proj.lora_B["a"].normal_()
        state = adapter_state_dict(m, "a")
        add_adapter(m, "c")
        load_adapter_state_dict(m, "c", state)
        torch.testing.assert_close(m.q_proj.lora_A["a"], m.q_proj.lora_A["c"])

    def test_save_load_dir(self, tmp_path):
        from agilerl_amd.llm import load_adapter, save_adapter

        m = self._model()
        apply_lora(m, LoraConfig(r=4, target_modules=["q_proj"]), adapters=["a"])
        with torch.no_grad():
            m.q_proj.lora_B["a"].normal_()
        save_adapter(m, "a", str(tmp_path / "ad"))
        assert (tmp_path / "ad" / "adapter_model.safetensors").exists()
        assert (tmp_path / "ad" / "adapter_config.json").exists()
        m2 = self._model()
        apply_lora(m2, LoraConfig(r=4, target_modules=["q_proj"]), adapters=["a"])
        load_adapter(m2, "a", str(tmp_path / "ad"))
        torch.testing.assert_close(m.q_proj.lora_B["a"], m2.q_proj.lora_B["a"])


class TestFusedLogprobs:
    def test_matches_naive(self):
        N, H, V = 37, 16, 50
        hidden = torch.randn(N, H, requires_grad=True)
        weight = torch.randn(V, H, requires_grad=True)
        targets = torch.randint(0, V, (N,))
        lp = fused_linear_logprobs(hidden, weight, targets, chunk_rows=8)
        logits = hidden @ weight.t()
        ref = torch.log_softmax(logits, -1).gather(1, targets.unsqueeze(1)).squeeze(1)
        torch.testing.assert_close(lp, ref, rtol=1e-4, atol=1e-5)

    def test_backward_matches(self):
        N, H, V = 21, 8, 30
        hidden = torch.randn(N, H, requires_grad=True)
        weight = torch.randn(V, H, requires_grad=True)
        targets = torch.randint(0, V, (N,))
        g = torch.randn(N)
        lp = fused_linear_logprobs(hidden, weight, targets, chunk_rows=7)
        gh, gw = torch.autograd.grad(lp, [hidden, weight], g)
        h2 = hidden.detach().requires_grad_(True)
        w2 = weight.detach().requires_grad_(True)
        ref = torch.log_softmax(h2 @ w2.t(), -1).gather(1, targets.unsqueeze(1)).squeeze(1)
        rgh, rgw = torch.autograd.grad(ref, [h2, w2], g)
        torch.testing.assert_close(gh, rgh, rtol=1e-4, atol=1e-5)
        torch.testing.assert_close(gw, rgw, rtol=1e-4, atol=1e-5)

    def test_temperature(self):
        N, H, V = 8, 8, 20
        hidden = torch.randn(N, H)
        weight = torch.randn(V, H)
        targets = torch.randint(0, V, (N,))
        lp = fused_linear_logprobs(hidden, weight, targets, temperature=2.0)
        ref = torch.log_softmax(hidden @ weight.t() / 2.0, -1).gather(1, targets.unsqueeze(1)).squeeze(1)
        torch.testing.assert_close(lp, ref, rtol=1e-4, atol=1e-5)


class TestGrpoLoss:
    def test_grad_direction(self):
        torch.manual_seed(0)
        logp = torch.randn(4, 6, requires_grad=True)
        old = logp.detach() + 0.01 * torch.randn(4, 6)
        adv = torch.ones(4, 6)
        mask = torch.ones(4, 6)
        loss = grpo_policy_loss(logp, old, adv, mask)
        (g,) = torch.autograd.grad(loss, logp)
        # positive advantage -> gradient pushes logp UP (negative grad of loss)
        assert (g < 0).all()

    def test_sequence_norm(self):
        logp = torch.zeros(2, 4, requires_grad=True)
        old = torch.zeros(2, 4)
        adv = torch.ones(2, 4)
        mask = torch.tensor([[1.0, 1, 1, 1], [1, 0, 0, 0]])
        l_tok = grpo_policy_loss(logp, old, adv, mask, loss_norm="token")
        l_seq = grpo_policy_loss(logp, old, adv, mask, loss_norm="sequence")
        assert float(l_tok.detach()) == pytest.approx(-1.0)
        assert float(l_seq.detach()) == pytest.approx(-1.0)


class TestGRPOAgent:
    def test_generate_and_learn(self):
        from agilerl_amd.algorithms.llm.grpo import GRPO
        from agilerl_amd.llm_envs import TokenReasoningGym, make_grpo_experiences

        agent = tiny_agent(GRPO, group_size=4, lr=1e-3, beta=0.04, max_completion_tokens=8)
        env = TokenReasoningGym(vocab_size=128, prompt_len=8, data_batch_size=2, group_size=4, seed=0)
        prompts = env.reset()
        seqs = agent.get_action(prompts)
        assert seqs.shape[0] == 8 and seqs.shape[1] > 8
        rewards = env.score(seqs)
        exp = make_grpo_experiences(env, seqs, rewards)
        stats = agent.learn(exp)
        assert np.isfinite(stats["loss"])
        assert stats["kl"] >= -1e-5

    def test_clone_shares_base_and_copies_adapter(self):
        from agilerl_amd.algorithms.llm.grpo import GRPO

        agent = tiny_agent(GRPO)
        clone = agent.clone(index=1)
        assert clone.model is agent.model
        assert clone.adapter_name != agent.adapter_name
        s1 = adapter_state_dict(agent.model, agent.adapter_name)
        s2 = adapter_state_dict(agent.model, clone.adapter_name)
        for k in s1:
            torch.testing.assert_close(s1[k], s2[k])

    def test_population_and_cleanup(self):
        from agilerl_amd.algorithms.llm.grpo import GRPO

        pop = GRPO.population(3, model_config=dict(TINY), dtype=torch.float32,
                              lora_config={"r": 4}, group_size=2)
        assert all(p.model is pop[0].model for p in pop)
        names = {p.adapter_name for p in pop}
        assert len(names) == 3
        pop[2].clean_up()
        from agilerl_amd.llm.lora import iter_lora_modules

        for _, mod in iter_lora_modules(pop[0].model):
            assert pop[2].adapter_name not in mod.lora_A

    def test_checkpoint_dir(self, tmp_path):
        from agilerl_amd.algorithms.llm.grpo import GRPO

        agent = tiny_agent(GRPO)
        with torch.no_grad():
            for p in agent.policy_network.parameters():
                p.normal_()
        path = str(tmp_path / "llm_ckpt")
        agent.save_checkpoint(path)
        import os

        assert os.path.exists(os.path.join(path, "actor", "adapter_model.safetensors"))
        agent2 = tiny_agent(GRPO)
        agent2.load_checkpoint(path)
        s1 = adapter_state_dict(agent.model, agent.adapter_name)
        s2 = adapter_state_dict(agent2.model, agent2.adapter_name)
        for k in s1:
            torch.testing.assert_close(s1[k], s2[k])

    def test_cispo_and_gspo(self):
        from agilerl_amd.algorithms.llm.cispo import CISPO
        from agilerl_amd.algorithms.llm.gspo import GSPO
        from agilerl_amd.llm_envs import TokenReasoningGym, make_grpo_experiences

        for cls in (CISPO, GSPO):
            agent = tiny_agent(cls, group_size=2, max_completion_tokens=4)
            env = TokenReasoningGym(vocab_size=128, prompt_len=6, data_batch_size=2, group_size=2)
            prompts = env.reset()
            seqs = agent.get_action(prompts)
            exp = make_grpo_experiences(env, seqs, env.score(seqs))
            stats = agent.learn(exp)
            assert np.isfinite(stats["loss"])


class TestSFTAndDPO:
    def test_sft_reduces_loss(self):
        from agilerl_amd.algorithms.llm.sft import SFT
        from agilerl_amd.llm_envs import SyntheticSFTGym

        agent = tiny_agent(SFT, lr=5e-3)
        env = SyntheticSFTGym(vocab_size=128, prompt_len=6, completion_len=6,
                              data_batch_size=8, seed=0)
        first = agent.learn(env.sample())["loss"]
        for _ in range(15):
            last = agent.learn(env.sample())["loss"]
        assert last < first

    def test_dpo_margin_grows(self):
        from agilerl_amd.algorithms.llm.dpo import DPO
        from agilerl_amd.llm_envs import SyntheticPreferenceGym

        agent = tiny_agent(DPO, lr=5e-3, beta=0.5)
        env = SyntheticPreferenceGym(vocab_size=128, prompt_len=6, completion_len=6,
                                     data_batch_size=8, seed=0)
        for _ in range(10):
            stats = agent.learn(env.sample())
        assert stats["margin"] > 0
        acc = agent.test(env)
        assert acc > 0.5


class TestLLMTrainingLoop:
    def test_reasoning_loop_with_evolution(self):
        from agilerl_amd.algorithms.llm.grpo import GRPO
        from agilerl_amd.hpo import Mutations, TournamentSelection
        from agilerl_amd.llm_envs import TokenReasoningGym
        from agilerl_amd.training.llm import finetune_llm_reasoning

        pop = GRPO.population(2, model_config=dict(TINY), dtype=torch.float32,
                              lora_config={"r": 4}, group_size=2,
                              max_completion_tokens=4, lr=1e-3)
        env = TokenReasoningGym(vocab_size=128, prompt_len=6, data_batch_size=2, group_size=2)
        agents, hist = finetune_llm_reasoning(
            env, pop, max_steps=4, evo_steps=2, eval_loop=1,
            tournament=TournamentSelection(2, True),
            mutation=Mutations(no_mutation=0.5, architecture=0.0, parameters=0.0,
                               activation=0.0, rl_hp=0.5, rand_seed=0),
            verbose=False,
        )
        assert len(agents) == 2
        assert len(hist) >= 1

    def test_llm_manifest(self):
        from agilerl_amd.training.trainer import LocalTrainer

        m = {
            "algorithm": {"name": "GRPO", "hyperparameters": {
                "model_config": dict(TINY), "dtype": "float32",
                "lora_config": {"r": 4}, "group_size": 2,
                "max_completion_tokens": 4, "lr": 1e-3,
            }},
            "environment": {"type": "llm", "env_type": "reasoning",
                            "data_batch_size": 2, "group_size": 2, "max_prompt_tokens": 6},
            "training": {"max_steps": 2, "pop_size": 1, "evo_steps": 1},
        }
        # dtype strings resolve in the trainer path
        m["algorithm"]["hyperparameters"]["dtype"] = torch.float32
        agents, hist = LocalTrainer.from_manifest(m).train()
        assert agents[0].algo == "GRPO"


class TestMultiTurn:
    def test_sync_vec_env_trajectories(self):
        from agilerl_amd.llm_envs.multiturn import SyncMultiTurnVecEnv, TokenGuessEnv

        env = SyncMultiTurnVecEnv(lambda: TokenGuessEnv(128, prompt_len=6, max_turns=2),
                                  data_batch_size=2, group_size=2, max_turns=2, seed=0)
        prompts = env.reset()
        assert prompts["input_ids"].shape[0] == 4
        # fake completions: 3 tokens each turn
        fake = torch.cat([prompts["input_ids"],
                          torch.randint(1, 128, (4, 3))], dim=1)
        prompts2, done = env.step(fake)
        assert not done and prompts2["input_ids"].shape[1] > prompts["input_ids"].shape[1]
        fake2 = torch.cat([prompts2["input_ids"], torch.randint(1, 128, (4, 3))], dim=1)
        _, done = env.step(fake2)
        assert done
        traj = env.get_trajectories()
        assert traj["action_mask"].sum() > 0
        assert traj["turn_ids"].max() == 1
        assert traj["rewards"].shape == (4,)

    def test_multiturn_rollout_and_learn(self):
        from agilerl_amd.algorithms.llm.grpo import GRPO
        from agilerl_amd.llm_envs.multiturn import SyncMultiTurnVecEnv, TokenGuessEnv
        from agilerl_amd.training.llm.multiturn import rollout_multiturn

        agent = tiny_agent(GRPO, group_size=2, max_completion_tokens=4, lr=1e-3)
        env = SyncMultiTurnVecEnv(lambda: TokenGuessEnv(128, prompt_len=6, max_turns=2),
                                  data_batch_size=2, group_size=2, max_turns=2, seed=0)
        traj = rollout_multiturn(agent, env)
        stats = agent.learn(traj)
        assert np.isfinite(stats["loss"])

    def test_multiturn_loop(self):
        from agilerl_amd.algorithms.llm.grpo import GRPO
        from agilerl_amd.hpo import Mutations, TournamentSelection
        from agilerl_amd.llm_envs.multiturn import SyncMultiTurnVecEnv, TokenGuessEnv
        from agilerl_amd.training.llm.multiturn import finetune_llm_multiturn

        pop = GRPO.population(2, model_config=dict(TINY), dtype=torch.float32,
                              lora_config={"r": 4}, group_size=2,
                              max_completion_tokens=4, lr=1e-3)
        env = SyncMultiTurnVecEnv(lambda: TokenGuessEnv(128, prompt_len=6, max_turns=2),
                                  data_batch_size=2, group_size=2, max_turns=2, seed=0)
        agents, hist = finetune_llm_multiturn(
            env, pop, max_steps=2, evo_steps=1,
            tournament=TournamentSelection(2, True),
            mutation=Mutations(no_mutation=0.5, architecture=0, parameters=0,
                               activation=0, rl_hp=0.5, rand_seed=0),
            verbose=False)
        assert len(hist) >= 1


class TestPPOLLMAndReinforce:
    def test_ppollm_learn_and_clone(self):
        from agilerl_amd.algorithms.llm.ppo_llm import PPOLLM
        from agilerl_amd.llm_envs import TokenReasoningGym, make_grpo_experiences

        agent = tiny_agent(PPOLLM, lr=1e-3, max_completion_tokens=4)
        env = TokenReasoningGym(vocab_size=128, prompt_len=6, data_batch_size=4, group_size=1, seed=0)
        p = env.reset()
        seqs = agent.get_action(p)
        stats = agent.learn(make_grpo_experiences(env, seqs, env.score(seqs)))
        assert np.isfinite(stats["loss"]) and np.isfinite(stats["value_loss"])
        clone = agent.clone(1)
        assert clone.value_head is not agent.value_head
        torch.testing.assert_close(
            clone.value_head.weight, agent.value_head.weight
        )

    def test_reinforce_rloo_advantage(self):
        from agilerl_amd.algorithms.llm.reinforce_llm import ReinforceLLM

        agent = tiny_agent(ReinforceLLM, group_size=4, max_completion_tokens=4)
        r = torch.tensor([1.0, 0.0, 0.0, 0.0])
        adv = agent._calculate_advantages(r)
        # RLOO: a_0 = r_0 - mean(others) = 1 - 0 = 1
        assert adv[0].item() == pytest.approx(1.0, abs=1e-5)
        assert adv[1].item() == pytest.approx(-1.0 / 3.0, abs=1e-5)


class TestLLMUtils:
    def test_packing_roundtrip(self):
        from agilerl_amd.llm import pack_padded_batch, unpack_values

        ids = torch.tensor([[5, 6, 7, 0, 0], [8, 9, 0, 0, 0]])
        am = (ids != 0).long()
        pack = pack_padded_batch(ids, am)
        assert pack["packed_ids"].tolist() == [[5, 6, 7, 8, 9]]
        assert pack["position_ids"].tolist() == [[0, 1, 2, 0, 1]]
        assert pack["cu_seqlens"].tolist() == [0, 3, 5]
        vals = torch.tensor([1.0, 2.0, 3.0, 4.0, 5.0])
        unpacked = unpack_values(vals, pack)
        assert unpacked[0].tolist() == [1.0, 2.0, 3.0, 0.0, 0.0]
        assert unpacked[1].tolist() == [4.0, 5.0, 0.0, 0.0, 0.0]

    def test_warmup_cosine(self):
        from agilerl_amd.llm import create_warmup_cosine_scheduler

        opt = torch.optim.AdamW([torch.nn.Parameter(torch.zeros(1))], lr=1.0)
        sched = create_warmup_cosine_scheduler(opt, total_steps=100, warmup_ratio=0.1)
        lrs = []
        for _ in range(100):
            lrs.append(opt.param_groups[0]["lr"])
            opt.step()
            sched.step()
        assert lrs[0] < 0.2           # warmup starts low
        assert abs(lrs[10] - 1.0) < 0.05  # peak after warmup
        assert lrs[-1] < 0.25          # decayed toward min ratio

    def test_create_population_util(self):
        from agilerl_amd.spaces import Box, Discrete
        from agilerl_amd.utils import create_population

        pop = create_population("DQN", Box(-1, 1, (4,)), Discrete(2),
                                population_size=3, INIT_HP={"batch_size": 32})
        assert len(pop) == 3 and pop[0].batch_size == 32


class TestSearchAndFormat:
    def test_search_tool(self):
        from agilerl_amd.llm_envs import SearchTool

        tool = SearchTool(["the cat sat", "dogs bark loudly", "cats and dogs"])
        hits = tool("cat dogs", k=2)
        assert len(hits) >= 1
        assert any("cat" in h or "dogs" in h for h in hits)

    def test_format_reward(self):
        from agilerl_amd.llm_envs import FormatRewardWrapper

        base = lambda c, a: 1.0 if c == a else 0.0
        fn = FormatRewardWrapper(base, format_bonus=0.1)
        assert fn("<answer>42</answer>", "42") == pytest.approx(1.1)
        assert fn("42", "42") == pytest.approx(1.0)  # fallback to raw
        strict = FormatRewardWrapper(base, require_format=True)
        assert strict("42", "42") == 0.0

    def test_from_dataset(self):
        from datasets import Dataset

        from agilerl_amd.llm_envs import HuggingFaceGym, ReasoningGym

        # HuggingFaceGym is now the dataset-backed class (no longer an
        # alias of ReasoningGym); both support dataset construction

        class TinyTok:
            pad_token_id = 0
            pad_token = "<pad>"
            eos_token = "<eos>"
            chat_template = None

            def __call__(self, texts, **kw):
                ids = [[(hash(w) % 99) + 1 for w in t.split()][:6] for t in texts]
                L = max(len(i) for i in ids)
                out = torch.zeros(len(ids), L, dtype=torch.long)
                am = torch.zeros(len(ids), L, dtype=torch.long)
                for j, i in enumerate(ids):
                    out[j, L - len(i):] = torch.tensor(i)
                    am[j, L - len(i):] = 1
                return {"input_ids": out, "attention_mask": am}

            def batch_decode(self, seqs, **kw):
                return [" ".join(str(int(t)) for t in s if t) for s in seqs]

        ds = Dataset.from_dict({"question": ["a b", "c d"], "answer": ["x", "y"]})
        gym = ReasoningGym.from_dataset(ds, lambda c, a: 0.5, TinyTok(),
                                        data_batch_size=2, group_size=2)
        p = gym.reset()
        assert p["input_ids"].shape[0] == 4
        seqs = torch.cat([p["input_ids"], torch.randint(1, 99, (4, 2))], dim=1)
        assert (gym.score(seqs) == 0.5).all()


class TestAdapterCleanupOnEvolve:
    def test_distributed_population_frees_adapters(self):
        from agilerl_amd.algorithms.llm.grpo import GRPO
        from agilerl_amd.hpo import TournamentSelection
        from agilerl_amd.llm.lora import iter_lora_modules
        from agilerl_amd.parallel import DistributedPopulation

        pop_agents = GRPO.population(3, model_config=dict(TINY), dtype=torch.float32,
                                     lora_config={"r": 4}, group_size=2)
        model = pop_agents[0].model
        dp = DistributedPopulation.__new__(DistributedPopulation)
        from agilerl_amd.parallel import DistributedState

        dp.state = DistributedState(0, 0, 1, "none", "cpu")
        dp.pop_size = 3
        dp.agent_factory = None
        dp.agents = {i: a for i, a in enumerate(pop_agents)}
        dp.local_indices = [0, 1, 2]
        dp.evo_step = 0
        for i, a in dp.agents.items():
            a.fitness.append(float(i))
        dp.evolve(TournamentSelection(3, True, rng=__import__("numpy").random.default_rng(0)))
        n_adapters = len(next(iter_lora_modules(model))[1].lora_A)
        assert n_adapters == 3  # exactly pop_size slots remain (no leak)


class TestPacking:
    def test_packed_logprobs_match_padded(self):
        torch.manual_seed(0)
        from agilerl_amd.algorithms.llm.grpo import GRPO

        agent = tiny_agent(GRPO)
        B, T = 3, 12
        ids = torch.randint(1, 128, (B, T))
        mask = torch.ones(B, T, dtype=torch.long)
        mask[0, :5] = 0
        ids[0, :5] = 0
        mask[2, :2] = 0
        ids[2, :2] = 0
        lp = agent.compute_logprobs(ids, mask)
        lpp = agent.compute_logprobs_packed(ids, mask)
        real = (mask[:, 1:] * mask[:, :-1]).bool()
        torch.testing.assert_close(lp[real], lpp[real], atol=1e-4, rtol=1e-4)
        # pad targets are zeroed in the packed output
        assert (lpp[~real] == 0).all()

    def test_grpo_learn_with_packing(self):
        torch.manual_seed(0)
        from agilerl_amd.algorithms.llm.grpo import GRPO
        from agilerl_amd.llm_envs import TokenReasoningGym, make_grpo_experiences

        agent = tiny_agent(GRPO, group_size=4, lr=1e-3, beta=0.04,
                           max_completion_tokens=6, use_packing=True)
        env = TokenReasoningGym(vocab_size=128, prompt_len=6, data_batch_size=2,
                                group_size=4, seed=0)
        prompts = env.reset()
        seqs = agent.get_action(prompts)
        exp = make_grpo_experiences(env, seqs, env.score(seqs))
        stats = agent.learn(exp)
        assert np.isfinite(stats["loss"])
        assert stats["kl"] >= -1e-5


def test_sft_packed_matches_padded_loss():
    torch.manual_seed(0)
    from agilerl_amd.algorithms.llm.sft import SFT

    def mk(**kw):
        torch.manual_seed(0)
        return tiny_agent(SFT, lr=1e-3, **kw)

    a1, a2 = mk(), mk(use_packing=True)
    B, T = 4, 12
    ids = torch.randint(1, 128, (B, T))
    mask = torch.ones(B, T, dtype=torch.long)
    mask[0, :5] = 0
    ids[0, :5] = 0
    amask = torch.zeros(B, T - 1)
    amask[:, 6:] = 1.0
    amask[0, : 5] = 0.0
    l1 = a1.learn({"ids": ids, "attention_mask": mask, "action_mask": amask})
    l2 = a2.learn({"ids": ids, "attention_mask": mask, "action_mask": amask})
    assert abs(l1["loss"] - l2["loss"]) < 1e-4


def test_dpo_packed_matches_padded_loss():
    from agilerl_amd.algorithms.llm.dpo import DPO

    def mk(**kw):
        torch.manual_seed(0)
        return tiny_agent(DPO, lr=1e-3, beta=0.1, **kw)

    a1, a2 = mk(), mk(use_packing=True)
    B, T = 4, 10
    c_ids = torch.randint(1, 128, (B, T))
    r_ids = torch.randint(1, 128, (B, T))
    c_am = torch.ones(B, T, dtype=torch.long)
    c_am[1, :3] = 0
    c_ids[1, :3] = 0
    r_am = torch.ones(B, T, dtype=torch.long)
    cm = torch.zeros(B, T - 1); cm[:, 4:] = 1.0
    rm = torch.zeros(B, T - 1); rm[:, 4:] = 1.0
    exp = {"chosen_ids": c_ids, "rejected_ids": r_ids,
           "chosen_attention_mask": c_am, "rejected_attention_mask": r_am,
           "chosen_mask": cm, "rejected_mask": rm}
    l1 = a1.learn(dict(exp))
    l2 = a2.learn(dict(exp))
    assert abs(l1["loss"] - l2["loss"]) < 1e-4
    assert abs(l1["margin"] - l2["margin"]) < 1e-3


class _WordTok:
    """Reversible word-level tokenizer for text-env tests (offline)."""

    chat_template = None
    pad_token_id = 0

    def __init__(self):
        self.vocab = {}
        self.words = []

    def encode(self, text):
        out = []
        for w in text.split():
            if w not in self.vocab:
                self.vocab[w] = len(self.words) + 1
                self.words.append(w)
            out.append(self.vocab[w])
        return out

    def decode(self, ids):
        return " ".join(
            self.words[int(i) - 1] if 0 < int(i) <= len(self.words) else "?"
            for i in ids
        )


class TestTextMultiTurn:
    def test_tool_call_parsing(self):
        from agilerl_amd.llm_envs.search import parse_tool_calls

        calls = parse_tool_calls("think <tool>capital of france</tool> more <tool>x</tool>")
        assert calls == ["capital of france", "x"]
        assert parse_tool_calls("no calls here") == []

    def test_search_qa_env_flow(self):
        import numpy as np

        from agilerl_amd.llm_envs import SearchQAEnv

        tok = _WordTok()
        env = SearchQAEnv(
            tok,
            documents=["paris is the capital of france", "berlin is in germany"],
            questions=["what is the capital of france"],
            answers=["paris"],
            max_turns=2,
        )
        rng = np.random.default_rng(0)
        prompt = env.initial_prompt(rng)
        assert "what is the capital" in tok.decode(prompt)  # chat-template framing around it
        # turn 0: a tool call gets search results + small format bonus
        call = tok.encode("<tool>capital france</tool>")
        feedback, r, done = env.respond(0, call, rng)
        assert not done and r == 0.05
        assert "paris" in tok.decode(feedback)
        # final turn: correct answer scores 1
        ans = tok.encode("<answer>paris</answer>")
        _, r, done = env.respond(1, ans, rng)
        assert done and r == 1.0
        # wrong answer scores 0
        env.initial_prompt(rng)
        _, r, done = env.respond(1, tok.encode("<answer>berlin</answer>"), rng)
        assert done and r == 0.0

    def test_text_env_through_sync_vec_env(self):
        import numpy as np

        from agilerl_amd.llm_envs import SearchQAEnv, SyncMultiTurnVecEnv

        tok = _WordTok()
        # pre-seed vocab so the env's encodes are stable across factories
        factory = lambda: SearchQAEnv(
            tok, documents=["paris is the capital of france"],
            questions=["capital of france ?"], answers=["paris"], max_turns=2,
        )
        venv = SyncMultiTurnVecEnv(factory, data_batch_size=2, group_size=2,
                                   max_turns=2, seed=0)
        obs = venv.reset()
        assert obs["input_ids"].shape[0] == 4


class TestGrpoParityDeepening:
    """Round-2 parity: IS levels, loss-norm variants, turn advantages,
    sampling-IS correction (reference grpo.py:1848-1903, 1619-1694,
    2500-2510, 1250-1379)."""

    def _tiny_agent(self, **kw):
        from agilerl_amd.algorithms.llm.grpo import GRPO

        tiny = dict(model_type="llama", vocab_size=64, hidden_size=32,
                    intermediate_size=64, num_hidden_layers=1,
                    num_attention_heads=2, num_key_value_heads=1,
                    max_position_embeddings=128, pad_token_id=0)
        torch.manual_seed(0)
        kw.setdefault("micro_batch_size", 2)
        return GRPO(model_config=tiny, dtype=torch.float32, lora_config={"r": 2},
                    group_size=2, **kw)

    def _batch(self, B=4, T=12, turns=False):
        g = torch.Generator().manual_seed(3)
        ids = torch.randint(1, 64, (B, T), generator=g)
        pos = torch.arange(T - 1).unsqueeze(0)
        action_mask = (pos + 1 >= T // 2).float().expand(B, T - 1)
        out = {"ids": ids, "action_mask": action_mask,
               "rewards": torch.rand(B, generator=g)}
        if turns:
            # two turns over the completion half
            tid = torch.full((B, T - 1), -1, dtype=torch.long)
            half = (T - 1 + T // 2) // 2
            tid[:, T // 2 - 1: half] = 0
            tid[:, half:] = 1
            out["turn_ids"] = tid
            out["turn_rewards"] = torch.rand(B, 2, generator=g)
        return out

    def test_is_levels_run_and_differ(self):
        losses = {}
        for level in ("token", "turn", "trajectory"):
            agent = self._tiny_agent(importance_sampling_level=level,
                                     update_epochs=2)
            stats = agent.learn(self._batch(turns=True))
            losses[level] = stats["loss"]
            assert np.isfinite(stats["loss"])
        # epoch 2 ratios != 1, so pooled levels give different losses
        assert losses["token"] != losses["trajectory"]

    def test_gspo_uses_trajectory_level(self):
        from agilerl_amd.algorithms.llm.gspo import GSPO

        tiny = dict(model_type="llama", vocab_size=64, hidden_size=32,
                    intermediate_size=64, num_hidden_layers=1,
                    num_attention_heads=2, num_key_value_heads=1,
                    max_position_embeddings=128, pad_token_id=0)
        agent = GSPO(model_config=tiny, dtype=torch.float32, lora_config={"r": 2},
                     group_size=2)
        assert agent.importance_sampling_level == "trajectory"
        stats = agent.learn(self._batch())
        assert np.isfinite(stats["loss"])

    def test_turn_level_advantages(self):
        agent = self._tiny_agent(advantage_level="turn")
        batch = self._batch(turns=True)
        adv = agent._turn_advantages(
            batch["turn_rewards"], batch["turn_ids"], batch["action_mask"])
        assert adv.shape == batch["action_mask"].shape
        # non-action targets carry zero advantage
        assert (adv * (1 - batch["action_mask"])).abs().sum() == 0
        # group-centered: within each prompt group and turn, advantages sum to ~0
        B = adv.shape[0]
        tr = batch["turn_rewards"].view(-1, 2, 2)
        centered = tr - tr.mean(dim=1, keepdim=True)
        assert abs(float(centered.view(B, 2).sum())) < 1e-4
        stats = agent.learn(batch)
        assert np.isfinite(stats["loss"])

    def test_sampling_is_correction_changes_loss(self):
        from agilerl_amd.ops.grpo_loss import grpo_policy_loss

        g = torch.Generator().manual_seed(1)
        B, T = 4, 10
        logp = torch.randn(B, T, generator=g) * 0.1 - 2
        old = logp + torch.randn(B, T, generator=g) * 0.05
        samp = old + torch.randn(B, T, generator=g) * 0.5
        adv = torch.randn(B, T, generator=g)
        mask = torch.ones(B, T)
        base = grpo_policy_loss(logp, old, adv, mask)
        corrected = grpo_policy_loss(logp, old, adv, mask, sampling_logp=samp,
                                     sampling_cap=2.0)
        assert float(base) != float(corrected)
        # cap: with sampling == old the ratio is 1 -> identical loss
        same = grpo_policy_loss(logp, old, adv, mask, sampling_logp=old)
        torch.testing.assert_close(same, base)

    def test_pool_log_ratio_turn_vs_trajectory(self):
        from agilerl_amd.ops.grpo_loss import pool_log_ratio

        g = torch.Generator().manual_seed(2)
        lr = torch.randn(2, 8, generator=g)
        mask = torch.ones(2, 8)
        traj = pool_log_ratio(lr, mask, None, "trajectory")
        torch.testing.assert_close(traj.squeeze(1), lr.mean(dim=1))
        tid = torch.tensor([[0, 0, 0, 0, 1, 1, 1, 1]] * 2)
        turn = pool_log_ratio(lr, mask, tid, "turn")
        torch.testing.assert_close(turn[:, 0], lr[:, :4].mean(dim=1))
        torch.testing.assert_close(turn[:, 5], lr[:, 4:].mean(dim=1))

    def test_accumulation_window_norm(self):
        agent = self._tiny_agent(loss_norm="accumulation_window",
                                 grad_accumulation_steps=2, micro_batch_size=2)
        stats = agent.learn(self._batch(B=4))
        assert np.isfinite(stats["loss"])

    def test_multiturn_env_emits_turn_rewards_and_sampling_logps(self):
        from agilerl_amd.llm_envs.multiturn import SyncMultiTurnVecEnv, TokenGuessEnv

        env = SyncMultiTurnVecEnv(lambda: TokenGuessEnv(vocab_size=32),
                                  data_batch_size=2, group_size=2, max_turns=2)
        prompts = env.reset()
        P = prompts["input_ids"].shape[1]
        done = False
        while not done:
            B, Pn = prompts["input_ids"].shape
            seqs = torch.cat([prompts["input_ids"],
                              torch.randint(1, 32, (B, 4))], dim=1)
            samp = torch.full((B, seqs.shape[1] - 1), -1.5)
            prompts, done = env.step(seqs, sampling_logps=samp)
        traj = env.get_trajectories()
        assert traj["turn_rewards"].shape == (4, 2)
        torch.testing.assert_close(
            traj["turn_rewards"].sum(dim=1), traj["rewards"])
        # sampling logps present exactly on action targets
        sl = traj["sampling_logps"]
        am = traj["action_mask"]
        assert sl.shape == am.shape
        assert ((sl != 0).float() * (1 - am)).sum() == 0
        assert float((sl * am).sum()) != 0.0

    def test_multiturn_learn_with_sampling_is(self):
        from agilerl_amd.llm_envs.multiturn import SyncMultiTurnVecEnv, TokenGuessEnv
        from agilerl_amd.training.llm.multiturn import rollout_multiturn

        agent = self._tiny_agent(sampling_is_correction=True,
                                 advantage_level="turn",
                                 importance_sampling_level="turn",
                                 generation="paged", max_completion_tokens=4)
        env = SyncMultiTurnVecEnv(lambda: TokenGuessEnv(vocab_size=60),
                                  data_batch_size=2, group_size=2, max_turns=2)
        traj = rollout_multiturn(agent, env)
        assert "sampling_logps" in traj
        assert float(traj["sampling_logps"].abs().sum()) > 0  # engine captured
        stats = agent.learn(traj)
        assert np.isfinite(stats["loss"])


def _word_tokenizer(corpus):
    """Real PreTrainedTokenizerFast trained offline on the corpus."""
    from tokenizers import Tokenizer, models, pre_tokenizers, trainers
    from transformers import PreTrainedTokenizerFast

    tok = Tokenizer(models.WordLevel(unk_token="<unk>"))
    tok.pre_tokenizer = pre_tokenizers.Whitespace()
    tok.train_from_iterator(
        corpus, trainers.WordLevelTrainer(special_tokens=["<pad>", "<unk>", "<eos>"])
    )
    return PreTrainedTokenizerFast(
        tokenizer_object=tok, pad_token="<pad>", eos_token="<eos>", unk_token="<unk>"
    )


class TestHuggingFaceGym:
    """Dataset-backed gym (reference HuggingFaceGym, llm_envs/base.py:93):
    real datasets.Dataset + real fast tokenizer, epoch dataloaders,
    train/test split, evaluation mode."""

    def _gym(self, **kw):
        from datasets import Dataset

        from agilerl_amd.llm_envs import HuggingFaceGym

        train = Dataset.from_dict({
            "question": [f"what is {i} plus {i}" for i in range(10)],
            "answer": [str(2 * i) for i in range(10)],
        })
        test = Dataset.from_dict({
            "question": ["what is one plus one"], "answer": ["2"],
        })
        corpus = list(train["question"]) + list(train["answer"])
        tokenizer = _word_tokenizer(corpus)

        def reward(completion, answer):
            return float(answer in completion)

        kw.setdefault("data_batch_size", 4)
        kw.setdefault("group_size", 2)
        return HuggingFaceGym(train, test, tokenizer, reward, **kw), tokenizer

    def test_epoch_iteration_and_shapes(self):
        gym, tokenizer = self._gym()
        batch = gym.reset()
        assert batch["input_ids"].shape[0] == 4 * 2  # batch x group
        assert batch["attention_mask"].shape == batch["input_ids"].shape
        # epochs advance after consuming the shard
        for _ in range(6):
            gym.reset()
        assert gym.num_epochs >= 2
        assert gym.dataset_size == {"train": 10, "test": 1}

    def test_score_with_real_tokenizer_round_trip(self):
        gym, tokenizer = self._gym(group_size=1, data_batch_size=2)
        batch = gym.reset()
        P = batch["input_ids"].shape[1]
        # append the CORRECT answers as completion tokens
        answers = gym._batch_answers
        comp = tokenizer(list(answers), return_tensors="pt", padding=True)["input_ids"]
        seqs = torch.cat([batch["input_ids"], comp], dim=1)
        rewards = gym.score(seqs)
        assert rewards.shape == (2,)
        assert (rewards == 1.0).all()  # decoded completions contain answers

    def test_evaluation_mode_uses_test_split(self):
        gym, _ = self._gym(data_batch_size=1, group_size=1)
        gym.eval(True)
        gym.reset()
        assert gym._batch_answers == ["2"]
        gym.eval(False)
        gym.reset()
        assert gym.evaluation_mode is False

    def test_reset_dataloaders_restarts_epochs(self):
        gym, _ = self._gym()
        for _ in range(8):
            gym.reset()
        assert gym.num_epochs > 0
        gym.reset(reset_dataloaders=True)
        assert gym.num_epochs == 0

    def test_grpo_trains_on_hf_gym(self):
        """End-to-end: tiny llama + real tokenizer vocabulary + dataset gym
        -> generate + score + learn (real-tokenizer flow)."""
        from agilerl_amd.algorithms.llm.grpo import GRPO
        from agilerl_amd.llm_envs.base import make_grpo_experiences

        gym, tokenizer = self._gym(group_size=2, data_batch_size=2)
        vocab = tokenizer.vocab_size + 8
        tiny = dict(model_type="llama", vocab_size=vocab, hidden_size=32,
                    intermediate_size=64, num_hidden_layers=1,
                    num_attention_heads=2, num_key_value_heads=1,
                    max_position_embeddings=128,
                    pad_token_id=tokenizer.pad_token_id)
        agent = GRPO(model_config=tiny, dtype=torch.float32, lora_config={"r": 2},
                     group_size=2, micro_batch_size=2, max_completion_tokens=4,
                     tokenizer=tokenizer)
        prompts = gym.reset()
        seqs = agent.get_action(prompts)
        rewards = gym.score(seqs)
        exp = make_grpo_experiences(gym, seqs, rewards,
                                    pad_token_id=tokenizer.pad_token_id)
        stats = agent.learn(exp)
        assert np.isfinite(stats["loss"])


class TestMergedGeneration:
    def test_merge_unmerge_bitwise_exact(self):
        import torch.nn as nn

        from agilerl_amd.llm.lora import LoraConfig, LoraLinear

        torch.manual_seed(0)
        base = nn.Linear(32, 16, bias=False)
        mod = LoraLinear(base, LoraConfig(r=4, lora_alpha=8), adapters=("a",))
        with torch.no_grad():
            mod.lora_B["a"].normal_(0, 0.1)
        before = base.weight.detach().clone()
        for _ in range(5):  # repeated cycles must not drift a single bit
            mod.merge_adapter("a")
            assert not torch.equal(base.weight, before)
            mod.unmerge_adapter()
            assert torch.equal(base.weight, before)

    def test_merged_forward_matches_adapter_forward(self):
        import torch.nn as nn

        from agilerl_amd.llm.lora import LoraConfig, LoraLinear

        torch.manual_seed(1)
        base = nn.Linear(64, 32, bias=False)
        mod = LoraLinear(base, LoraConfig(r=8, lora_alpha=16), adapters=("a",))
        with torch.no_grad():
            mod.lora_B["a"].normal_(0, 0.05)
        mod.active_adapter = "a"
        x = torch.randn(4, 64)
        ref = mod(x)
        mod.merge_adapter("a")
        merged = mod(x)  # adapter path suppressed; delta folded into W
        mod.unmerge_adapter()
        torch.testing.assert_close(merged, ref, rtol=1e-5, atol=1e-5)

    def test_generate_paged_merged_parity_and_restore(self):
        """Merged generation (default) produces the same greedy tokens as
        explicit unmerged generation, and the base weights are restored
        bitwise afterwards — even with a NONZERO adapter delta."""
        from agilerl_amd.algorithms.llm.grpo import GRPO
        from agilerl_amd.llm.lora import iter_lora_modules

        tiny = dict(model_type="llama", vocab_size=64, hidden_size=32,
                    intermediate_size=64, num_hidden_layers=2,
                    num_attention_heads=2, num_key_value_heads=1,
                    max_position_embeddings=128, pad_token_id=0)
        torch.manual_seed(0)
        agent = GRPO(model_config=tiny, dtype=torch.float32, lora_config={"r": 2},
                     max_completion_tokens=6, generation="paged")
        with torch.no_grad():  # give the adapter a real delta
            for _, m in iter_lora_modules(agent.model):
                m.lora_B[agent.adapter_name].normal_(0, 0.02)
        snapshot = {
            n: m.base.weight.detach().clone()
            for n, m in iter_lora_modules(agent.model)
        }
        torch.manual_seed(1)
        ids = torch.randint(1, 64, (3, 5))
        mask = torch.ones_like(ids)
        agent.merged_generation = True
        out_merged = agent.generate_paged(ids, mask, do_sample=False)
        # weights restored bitwise, engine dropped state cleanly
        for n, m in iter_lora_modules(agent.model):
            assert torch.equal(m.base.weight, snapshot[n]), n
            assert m._merged is None
        agent.merged_generation = False
        agent._decode_engine = None  # fresh engine for the unmerged pass
        out_adapter = agent.generate_paged(ids, mask, do_sample=False)
        torch.testing.assert_close(out_merged, out_adapter)


def _contains_answer_reward(completion, answer):
    return float(str(answer) in completion)


class TestDatasetManifestFlow:
    def test_trainer_runs_dataset_backed_reasoning(self, tmp_path):
        """Manifest `dataset:` + `reward_fn:` + `tokenizer_path` ->
        LocalTrainer builds a HuggingFaceGym and trains GRPO end to end
        (the reference HuggingFaceGym flow, llm_envs/base.py:93)."""
        from datasets import Dataset, DatasetDict

        from agilerl_amd.models.manifest import TrainingManifest
        from agilerl_amd.training.trainer import LocalTrainer

        train = Dataset.from_dict({
            "question": [f"what is {i} plus {i}" for i in range(8)],
            "answer": [str(2 * i) for i in range(8)],
        })
        dd = DatasetDict({"train": train, "test": train.select(range(2))})
        ds_dir = tmp_path / "ds"
        dd.save_to_disk(str(ds_dir))
        tok = _word_tokenizer(list(train["question"]) + list(train["answer"]))
        tok_dir = tmp_path / "tok"
        tok.save_pretrained(str(tok_dir))

        vocab = tok.vocab_size + 8
        manifest = TrainingManifest.model_validate({
            "algorithm": {
                "name": "GRPO",
                "hyperparameters": {
                    "model_config": {
                        "model_type": "llama", "vocab_size": vocab,
                        "hidden_size": 32, "intermediate_size": 64,
                        "num_hidden_layers": 1, "num_attention_heads": 2,
                        "num_key_value_heads": 1,
                        "max_position_embeddings": 128,
                        "pad_token_id": tok.pad_token_id,
                    },
                    "lora_config": {"r": 2},
                    "dtype": "float32",
                    "group_size": 2,
                    "micro_batch_size": 2,
                    "max_completion_tokens": 4,
                },
            },
            "environment": {
                "type": "llm", "env_type": "reasoning",
                "dataset": str(ds_dir),
                "reward_fn": "tests.test_llm._contains_answer_reward",
                "data_batch_size": 2, "group_size": 2,
                "max_prompt_tokens": 16,
                "env_kwargs": {"tokenizer_path": str(tok_dir)},
            },
            "training": {"max_steps": 2, "pop_size": 2, "evo_steps": 1},
        })
        trainer = LocalTrainer(manifest, device="cpu")
        results = trainer.train()
        assert results is not None


class TestPpoLlmSamplingIs:
    def test_ppollm_consumes_sampling_logps(self):
        from agilerl_amd.algorithms.llm.ppo_llm import PPOLLM

        tiny = dict(model_type="llama", vocab_size=64, hidden_size=32,
                    intermediate_size=64, num_hidden_layers=1,
                    num_attention_heads=2, num_key_value_heads=1,
                    max_position_embeddings=128, pad_token_id=0)
        torch.manual_seed(0)
        agent = PPOLLM(model_config=tiny, dtype=torch.float32,
                       lora_config={"r": 2}, group_size=2, micro_batch_size=2,
                       sampling_is_correction=True)
        g = torch.Generator().manual_seed(1)
        ids = torch.randint(1, 64, (4, 12), generator=g)
        pos = torch.arange(11).unsqueeze(0)
        am = (pos + 1 >= 6).float().expand(4, 11)
        base = {"ids": ids, "action_mask": am, "rewards": torch.rand(4, generator=g)}
        stats = agent.learn({**base, "sampling_logps": torch.randn(4, 11, generator=g) - 2})
        assert np.isfinite(stats["loss"])


class TestReferenceLlmManifestFields:
    @pytest.mark.parametrize("cfg", [
        "grpo.yaml", "gspo.yaml", "cispo.yaml", "ppo_llm.yaml",
        "reinforce_llm.yaml", "ppo_llm_quant_bench.yaml",
    ])
    def test_reference_llm_yaml_constructs_with_local_overrides(self, tmp_path, cfg):
        """The actual reference LLM-finetuning YAMLs (vLLM-era fields,
        columns mapping, reward_file_path, train_test_split) run here with
        only a local model + dataset substituted for the hub entries."""
        import os
        import warnings

        import yaml as _yaml
        from datasets import Dataset

        from agilerl_amd.models.manifest import TrainingManifest
        from agilerl_amd.training.trainer import LocalTrainer

        ref = os.path.join(REF_CONFIGS, "llm_finetuning", cfg)
        doc = _yaml.safe_load(open(ref))

        # local stand-ins for the hub dataset/model (offline image)
        ds = Dataset.from_dict({
            "nums": [f"one plus {i}" for i in range(6)],
            "target": [str(i + 1) for i in range(6)],
        })
        ds_dir = tmp_path / "ds"
        ds.save_to_disk(str(ds_dir))
        (tmp_path / "reward.py").write_text(
            "def combined_rewards(completion, answer):\n"
            "    return float(str(answer) in completion)\n"
        )
        tok = _word_tokenizer(list(ds["nums"]) + list(ds["target"]))
        tok_dir = tmp_path / "tok"
        tok.save_pretrained(str(tok_dir))

        doc["environment"]["dataset"] = str(ds_dir)
        doc["environment"]["reward_file_path"] = str(tmp_path / "reward.py")
        doc["environment"].setdefault("env_kwargs", {})["tokenizer_path"] = str(tok_dir)
        doc["environment"]["max_prompt_tokens"] = 16
        doc["algorithm"]["model_config"] = {
            "model_type": "llama", "vocab_size": tok.vocab_size + 8,
            "hidden_size": 32, "intermediate_size": 64,
            "num_hidden_layers": 1, "num_attention_heads": 2,
            "num_key_value_heads": 1, "max_position_embeddings": 128,
            "pad_token_id": tok.pad_token_id,
        }
        doc["algorithm"]["lora_config"] = {"r": 2}
        doc["algorithm"]["dtype"] = "float32"
        doc["algorithm"]["max_completion_tokens"] = 4
        doc["algorithm"]["micro_batch_size"] = 2
        doc["training"].update({"max_steps": 2, "pop_size": 2, "evo_steps": 1})

        # reference puts algorithm kwargs at top level; fold into hyperparameters
        algo = doc["algorithm"]
        hp = {k: v for k, v in algo.items() if k != "name"}
        doc["algorithm"] = {"name": algo["name"], "hyperparameters": hp}

        manifest = TrainingManifest.model_validate(doc)
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            trainer = LocalTrainer(manifest, device="cpu")
            results = trainer.train()
        assert results is not None
        if cfg == "grpo.yaml":
            dropped = [str(x.message) for x in w
                       if "reference-only" in str(x.message)
                       or "paged-KV" in str(x.message)]
            assert dropped


class TestReferenceMultiturnManifest:
    @pytest.mark.parametrize("cfg", [
        "grpo_multiturn.yaml", "cispo_quant_bench.yaml",
        "reinforce_quant_bench.yaml", "cispo_gemma4_group5.yaml",
        "cispo_quant_bench_qwen.yaml",
    ])
    def test_reference_multiturn_yaml_runs(self, cfg):
        """The reference multiturn YAMLs train here: env_type routing to the
        multi-turn loop, game-env mapping (GuessTheNumber; unavailable GEM
        games warn and use the first-party stand-in), NETWORK-section
        lora_config, quantization fields warn-and-ignore — only the hub
        model is swapped for a local random-init config."""
        import os
        import yaml as _yaml

        from agilerl_amd.models.manifest import TrainingManifest
        from agilerl_amd.training.trainer import LocalTrainer

        ref = os.path.join(REF_CONFIGS, "llm_finetuning", cfg)
        doc = _yaml.safe_load(open(ref))
        algo = doc["algorithm"]
        hp = {k: v for k, v in algo.items() if k != "name"}
        hp.update({
            "model_config": {
                "model_type": "llama", "vocab_size": 64, "hidden_size": 32,
                "intermediate_size": 64, "num_hidden_layers": 1,
                "num_attention_heads": 2, "num_key_value_heads": 1,
                "max_position_embeddings": 256, "pad_token_id": 0,
            },
            "dtype": "float32", "max_completion_tokens": 4,
            "micro_batch_size": 2, "group_size": 2, "batch_size": 2,
        })
        doc["algorithm"] = {"name": algo["name"], "hyperparameters": hp}
        doc["environment"]["data_batch_size"] = 2
        doc["environment"]["group_size"] = 2
        doc["environment"]["max_turns"] = 2  # budget knob (quant configs use 50)
        doc["training"].update({"max_steps": 2, "pop_size": 2, "evo_steps": 1})
        manifest = TrainingManifest.model_validate(doc)
        trainer = LocalTrainer(manifest, device="cpu")
        results = trainer.train()
        assert results is not None


class TestGrpoReferenceSurface(TestGrpoParityDeepening):
    """Reference grpo.py:441-539 constructor surface: aliases, advantage
    post-processing, loss_type routing, schedules."""

    def test_aliases_map_to_native_options(self):
        import warnings

        with warnings.catch_warnings(record=True):
            warnings.simplefilter("always")
            a = self._tiny_agent(
                use_sequence_packing=False,
                vllm_importance_sampling_correction=True,
                vllm_importance_sampling_cap=3.0,
                micro_batch_size_per_gpu=1,
                action_granularity="turn",
                advantage_granularity="turn",
                max_output_tokens=33,
            )
        assert a.use_packing is False
        assert a.sampling_is_correction is True and a.sampling_is_cap == 3.0
        assert a.micro_batch_size == 1
        assert a.importance_sampling_level == "turn"
        assert a.advantage_level == "turn"
        assert a.max_completion_tokens == 33

    def test_loss_type_routing(self):
        assert self._tiny_agent(loss_type="cispo").CISPO is True
        assert self._tiny_agent(loss_type="gspo").importance_sampling_level == "trajectory"
        with pytest.raises(ValueError, match="loss_type"):
            self._tiny_agent(loss_type="bogus")

    def test_advantage_postprocessing(self):
        a = self._tiny_agent(whiten_advantages=True, adv_clip_range=0.5,
                             filter_zero_adv=True, adv_filter_eps=1e-6)
        stats = a.learn(self._batch())
        assert np.isfinite(stats["loss"])
        b = self._tiny_agent(adv_norm="mean_only")
        assert b.scale_rewards is False
        with pytest.raises(ValueError, match="adv_norm"):
            self._tiny_agent(adv_norm="bogus")

    def test_kl_advantage_shaping_needs_beta(self):
        a = self._tiny_agent(use_kl_advantage_shaping=True, beta=0.04)
        stats = a.learn(self._batch())
        assert np.isfinite(stats["loss"]) and stats["kl"] >= 0

    def test_cosine_schedule_steps(self):
        a = self._tiny_agent(
            cosine_lr_schedule_config={"num_epochs": 4, "warmup_proportion": 0.25})
        lr0 = a.optimizer.param_groups[0]["lr"]
        a.learn(self._batch())
        lr1 = a.optimizer.param_groups[0]["lr"]
        assert lr1 != lr0  # warmup/cosine moved the lr

    def test_ignored_infra_kwargs_warn_not_crash(self):
        import warnings

        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            a = self._tiny_agent(quantization_config={"bits": 4},
                                 reduce_memory_peak=True,
                                 lora_target_scope="all-linear")
        assert any("reference-only" in str(x.message) for x in w)
        assert np.isfinite(a.learn(self._batch())["loss"])

    def test_use_liger_loss_false_matches_fused_default(self):
        torch.manual_seed(0)
        a = self._tiny_agent(use_liger_loss=False)
        torch.manual_seed(0)
        b = self._tiny_agent()
        batch = self._batch()
        sa, sb = a.learn(batch), b.learn(batch)
        assert abs(sa["loss"] - sb["loss"]) < 1e-5  # CPU: both eager anyway


class TestSftDpoReferenceSurface:
    """Shared reference-kwarg resolver on SFT/DPO (reference sft.py /
    dpo.py constructor surfaces)."""

    def _tiny_cfg(self):
        return dict(model_type="llama", vocab_size=64, hidden_size=32,
                    intermediate_size=64, num_hidden_layers=1,
                    num_attention_heads=2, num_key_value_heads=1,
                    max_position_embeddings=128, pad_token_id=0)

    def test_sft_update_epochs_and_aliases(self):
        import warnings

        from agilerl_amd.algorithms.llm.sft import SFT

        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            a = SFT(model_config=self._tiny_cfg(), dtype=torch.float32,
                    lora_config={"r": 2}, model_name=None,
                    micro_batch_size_per_gpu=2, update_epochs=2, seed=3,
                    chunk_rows=64, quantization_config={"bits": 8})
        assert a.update_epochs == 2 and a.micro_batch_size == 2
        assert any("reference-only" in str(x.message) for x in w)
        g = torch.Generator().manual_seed(0)
        ids = torch.randint(1, 64, (4, 10), generator=g)
        mask = torch.ones(4, 9)
        out = a.learn({"ids": ids, "action_mask": mask})
        assert np.isfinite(out["loss"])

    def test_dpo_nll_alpha_changes_loss(self):
        from agilerl_amd.algorithms.llm.dpo import DPO

        g = torch.Generator().manual_seed(1)
        batch = {
            "chosen_ids": torch.randint(1, 64, (4, 10), generator=g),
            "rejected_ids": torch.randint(1, 64, (4, 10), generator=g),
            "chosen_mask": torch.ones(4, 9),
            "rejected_mask": torch.ones(4, 9),
        }
        torch.manual_seed(0)
        a = DPO(model_config=self._tiny_cfg(), dtype=torch.float32,
                lora_config={"r": 2}, nll_alpha=0.0)
        torch.manual_seed(0)
        b = DPO(model_config=self._tiny_cfg(), dtype=torch.float32,
                lora_config={"r": 2}, nll_alpha=0.5)
        la = a.learn({k: v.clone() for k, v in batch.items()})["loss"]
        lb = b.learn({k: v.clone() for k, v in batch.items()})["loss"]
        assert abs(la - lb) > 1e-6  # NLL term moved the loss

    def test_unknown_kwarg_still_raises(self):
        from agilerl_amd.algorithms.llm.sft import SFT

        with pytest.raises(TypeError, match="bogus"):
            SFT(model_config=self._tiny_cfg(), dtype=torch.float32,
                lora_config={"r": 2}, bogus_kwarg=1)


class TestPpoLlmTurnGae(TestGrpoParityDeepening):
    """Reference ppo_llm.py:1141 turn-level GAE: per-turn critic values,
    gamma/gae_lambda across turns, token broadcast via turn_ids."""

    def _tiny_ppo(self, **kw):
        from agilerl_amd.algorithms.llm.ppo_llm import PPOLLM

        tiny = dict(model_type="llama", vocab_size=64, hidden_size=32,
                    intermediate_size=64, num_hidden_layers=1,
                    num_attention_heads=2, num_key_value_heads=1,
                    max_position_embeddings=128, pad_token_id=0)
        torch.manual_seed(0)
        kw.setdefault("micro_batch_size", 2)
        return PPOLLM(model_config=tiny, dtype=torch.float32,
                      lora_config={"r": 2}, **kw)

    def test_multiturn_gae_learn(self):
        a = self._tiny_ppo(gamma=0.9, gae_lambda=0.8)
        batch = self._batch(turns=True)
        stats = a.learn(batch)
        assert np.isfinite(stats["loss"]) and np.isfinite(stats["value_loss"])

    def test_single_turn_unaffected(self):
        a = self._tiny_ppo()
        stats = a.learn(self._batch(turns=False))
        assert np.isfinite(stats["loss"])

    def test_turn_gae_math(self):
        """Hand-check the across-turn recursion on a 1-sample case."""
        a = self._tiny_ppo(gamma=0.5, gae_lambda=1.0)
        tr = torch.tensor([[1.0, 2.0]])
        tv = torch.tensor([[0.5, 0.25]])
        played = torch.ones(1, 2, dtype=torch.bool)
        adv = a._turn_gae(tr, tv, played)
        # t=1 (last): delta1 = 2 - 0.25 = 1.75
        # t=0: delta0 = 1 + 0.5*0.25 - 0.5 = 0.625; A0 = 0.625 + 0.5*1.75
        assert torch.allclose(adv, torch.tensor([[1.5, 1.75]]))

    def test_turn_aliases(self):
        a = self._tiny_ppo(turn_ratio_pooling=True, lr_actor=1e-5, lr_critic=1e-3)
        assert a.importance_sampling_level == "turn"
        assert a.lr == 1e-5
        assert a.value_optimizer.param_groups[0]["lr"] == 1e-3


class TestCollectRolloutsLlm(TestGrpoParityDeepening):
    def test_single_batch(self):
        from agilerl_amd.llm_envs import TokenReasoningGym
        from agilerl_amd.rollouts.on_policy import collect_rollouts_llm

        agent = self._tiny_agent(max_completion_tokens=8)
        env = TokenReasoningGym(vocab_size=64, prompt_len=8,
                                data_batch_size=2, group_size=2)
        exp, reward = collect_rollouts_llm(agent, env)
        assert {"ids", "action_mask", "rewards"} <= set(exp)
        stats = agent.learn(exp)
        assert np.isfinite(stats["loss"]) and np.isfinite(reward)

    def test_multi_batch(self):
        from agilerl_amd.llm_envs import TokenReasoningGym
        from agilerl_amd.rollouts.on_policy import collect_rollouts_llm

        agent = self._tiny_agent(max_completion_tokens=8)
        env = TokenReasoningGym(vocab_size=64, prompt_len=8,
                                data_batch_size=2, group_size=2)
        batches = collect_rollouts_llm(agent, env, n_batches=2)
        assert len(batches) == 2


class TestReferenceDpoManifest:
    def test_reference_dpo_yaml_with_local_preference_dataset(self, tmp_path):
        """The reference dpo.yaml trains against a local saved-to-disk
        preference dataset (prompt/chosen/rejected columns)."""
        import os

        import yaml as _yaml
        from datasets import Dataset

        from agilerl_amd.models.manifest import TrainingManifest
        from agilerl_amd.training.trainer import LocalTrainer

        ref = os.path.join(REF_CONFIGS, "llm_finetuning", "dpo.yaml")
        doc = _yaml.safe_load(open(ref))

        texts = [f"question {i}" for i in range(6)]
        ds = Dataset.from_dict({
            "prompt": texts,
            "chosen": [f"good answer {i}" for i in range(6)],
            "rejected": [f"bad {i}" for i in range(6)],
        })
        ds_dir = tmp_path / "prefds"
        ds.save_to_disk(str(ds_dir))
        tok = _word_tokenizer(texts + [f"good answer {i}" for i in range(6)]
                              + [f"bad {i}" for i in range(6)])
        tok_dir = tmp_path / "tok"
        tok.save_pretrained(str(tok_dir))

        doc["environment"]["dataset"] = str(ds_dir)
        doc["environment"].setdefault("env_kwargs", {})["tokenizer_path"] = str(tok_dir)
        doc["environment"]["data_batch_size"] = 2
        doc["algorithm"]["model_config"] = {
            "model_type": "llama", "vocab_size": tok.vocab_size + 8,
            "hidden_size": 32, "intermediate_size": 64,
            "num_hidden_layers": 1, "num_attention_heads": 2,
            "num_key_value_heads": 1, "max_position_embeddings": 128,
            "pad_token_id": tok.pad_token_id,
        }
        doc["algorithm"]["lora_config"] = {"r": 2}
        doc["algorithm"]["dtype"] = "float32"
        doc["algorithm"]["micro_batch_size"] = 2
        doc["training"].update({"max_steps": 2, "pop_size": 2, "evo_steps": 1})

        algo = doc["algorithm"]
        hp = {k: v for k, v in algo.items() if k != "name"}
        doc["algorithm"] = {"name": algo["name"], "hyperparameters": hp}

        manifest = TrainingManifest.model_validate(doc)
        trainer = LocalTrainer(manifest, device="cpu")
        results = trainer.train()
        assert results is not None


class TestReferenceSftManifest:
    def test_reference_sft_yaml_with_local_dataset(self, tmp_path):
        """The reference sft.yaml (response_column spelling) trains against
        a local saved-to-disk dataset."""
        import os

        import yaml as _yaml
        from datasets import Dataset

        from agilerl_amd.models.manifest import TrainingManifest
        from agilerl_amd.training.trainer import LocalTrainer

        ref = os.path.join(REF_CONFIGS, "sft.yaml")
        doc = _yaml.safe_load(open(ref))

        texts = [f"prompt {i}" for i in range(6)]
        ds = Dataset.from_dict({
            "prompt": texts,
            "chosen": [f"target {i}" for i in range(6)],
        })
        ds_dir = tmp_path / "sftds"
        ds.save_to_disk(str(ds_dir))
        tok = _word_tokenizer(texts + [f"target {i}" for i in range(6)])
        tok_dir = tmp_path / "tok"
        tok.save_pretrained(str(tok_dir))

        doc["environment"]["dataset"] = str(ds_dir)
        doc["environment"].setdefault("env_kwargs", {})["tokenizer_path"] = str(tok_dir)
        doc["environment"]["data_batch_size"] = 2
        doc["algorithm"]["model_config"] = {
            "model_type": "llama", "vocab_size": tok.vocab_size + 8,
            "hidden_size": 32, "intermediate_size": 64,
            "num_hidden_layers": 1, "num_attention_heads": 2,
            "num_key_value_heads": 1, "max_position_embeddings": 128,
            "pad_token_id": tok.pad_token_id,
        }
        doc["algorithm"]["lora_config"] = {"r": 2}
        doc["algorithm"]["dtype"] = "float32"
        doc["algorithm"]["micro_batch_size"] = 2
        doc["algorithm"]["gradient_checkpointing"] = False
        doc["training"].update({"max_steps": 2, "pop_size": 2, "evo_steps": 1})

        algo = doc["algorithm"]
        hp = {k: v for k, v in algo.items() if k != "name"}
        doc["algorithm"] = {"name": algo["name"], "hyperparameters": hp}

        manifest = TrainingManifest.model_validate(doc)
        trainer = LocalTrainer(manifest, device="cpu")
        results = trainer.train()
        assert results is not None
