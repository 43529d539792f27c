import os, warnings, torch, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from agilerl_amd.algorithms.ppo import PPO
from agilerl_amd.spaces import Box, Discrete

DEV = "cuda:0"

def flat(n=256, seed=1):
    g = torch.Generator().manual_seed(seed)
    return {
        "obs": torch.randn(n, 8, generator=g).to(DEV),
        "action": torch.randint(0, 4, (n,), generator=g).to(DEV),
        "log_prob": (torch.randn(n, generator=g) * 0.1).to(DEV),
        "advantages": torch.randn(n, generator=g).to(DEV),
        "returns": torch.randn(n, generator=g).to(DEV),
        "value": torch.randn(n, generator=g).to(DEV),
        "done": torch.zeros(n).to(DEV), "reward": torch.zeros(n).to(DEV),
    }

agents = []
for _ in range(2):
    torch.manual_seed(7)
    agents.append(PPO(Box(-1,1,(8,)), Discrete(4), batch_size=256, update_epochs=1,
                      device=DEV, net_config={"arch": "mlp", "hidden_size": [32, 32]}))
graphed, eager = agents
eager.target_kl = 1e9
graphed.learn(dict(flat()))
eager.learn(dict(flat()))
for tag, agent in (("graphed", graphed), ("eager", eager)):
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        try:
            agent.apply_architecture_mutation("encoder.add_node", numb_new_nodes=16)
        except Exception as e:
            print(tag, "RAISED:", type(e).__name__, e)
        for x in w:
            print(tag, "WARN:", x.category.__name__, str(x.message)[:300])
    print(tag, "shape:", tuple(agent.actor.encoder.model[0].weight.shape))
