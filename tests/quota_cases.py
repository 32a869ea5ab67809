"""What the quota-rule tests share (tests/test_eval_quota_host.py checks it without a GPU, tests/test_gpu_eval_quota.py rests
on it): the Breakout environments ``VectorEvaluator`` is evaluated over under the quota rule.  A positive step limit ends
every episode within ``episode_timestep_limit`` steps, so E episodes per stream end within the default cap of E x limit calls
under any policy: ``incomplete_streams == 0`` does not depend on what the agent does."""

QUOTA_ENV = dict(seed=0x5EEDFACE12345, kw=dict(sticky_action_prob=0.1, episode_timestep_limit=30), episodes=2)
