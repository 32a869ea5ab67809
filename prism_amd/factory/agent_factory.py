"""``build_agent(config, obs_shape, n_actions)`` — mirrors
``/root/reference/prism/factory/agent_factory.py:7-61``: online model, optional target model
(constructed second so it advances the torch RNG exactly as the reference does, then overwritten
with the online weights), action selectors, and the optimizer of the reference's three-way choice
(agent_factory.py:40-58: ``use_adam`` wins, then ``use_rmsprop``, else SGD), which ``HipAgent`` builds over its
flat parameter buffer (``hip_agent.build_optimizer``)."""
from prism_amd.agents import action_selectors, risk_policies
from prism_amd.agents.hip_agent import HipAgent
from prism_amd.factory import model_factory


def build_agent(config, obs_shape, n_actions, process_group=None):
    obs_shape = [int(a) for a in obs_shape]
    n_actions = int(n_actions)
    # two knobs that are not Config fields (config.py): which of the reference's IDS selectors trains, and whether the
    # evaluation selector is the reference's commented-out MinRegretActionSelector (agent_factory.py:29-30)
    ids_kind = getattr(config, "ids_action_selector", "ids")
    eval_kind = getattr(config, "eval_action_selector", "greedy")
    if ids_kind not in ("ids", "simple_ids"):
        raise ValueError(f"ids_action_selector must be 'ids' or 'simple_ids', got {ids_kind!r}")
    if eval_kind not in ("greedy", "min_regret"):
        raise ValueError(f"eval_action_selector must be 'greedy' or 'min_regret', got {eval_kind!r}")
    if not config.use_ids and (ids_kind != "ids" or eval_kind != "greedy"):
        raise ValueError("ids_action_selector = 'simple_ids' and eval_action_selector = 'min_regret' need use_ids")
    if ids_kind == "simple_ids" and config.ids_use_random_samples:
        raise ValueError("ids_action_selector = 'simple_ids' has no sampled form: ids_use_random_samples must be off "
                         "(the reference's SimpleIDSActionSelector raises on it)")
    # (an id the acting path cannot honour -- unknown name, eta missing or out of range, Q heads -- is refused before a model
    # is built)
    risk_policies.for_config(config)
    model = model_factory.create_model(obs_shape, n_actions, config)
    target_model = None
    if config.use_target_network:
        target_model = model_factory.create_model(obs_shape, n_actions, config)
        target_model.load_state_dict(model.state_dict())

    eval_selector = action_selectors.GreedyActionSelector()
    if config.use_ids:
        from prism_amd.agents import squish_functions
        _, unsquish = squish_functions.parse(config.loss_squish_fn_id)          # (agent_factory.py:20-27)
        ids_class = action_selectors.SimpleIDSActionSelector if ids_kind == "simple_ids" else action_selectors.IDSActionSelector
        selector = ids_class(config.ids_lambda, config.ids_use_random_samples, config.ids_epsilon,
                             config.ids_rho_lower_bound, config.ids_beta, unsquish)
        if eval_kind == "min_regret":
            eval_selector = action_selectors.MinRegretActionSelector(lmbda=config.ids_lambda, unsquish_function=unsquish)
    elif config.use_e_greedy:
        selector = action_selectors.EGreedyActionSelector(config.e_greedy_initial_epsilon,
                                                          config.e_greedy_final_epsilon,
                                                          config.e_greedy_decay_timesteps, config.seed)
    else:
        selector = action_selectors.GreedyActionSelector()
    return HipAgent(model, selector, eval_selector, target_model, config, obs_shape[-1], n_actions,
                    process_group=process_group)
