"""CPU: the log-prob consumers live once, in ``slnlp.judge.LogProbJudge``, and reach both estimators by inheritance."""
import pytest

CONSUMERS = ("predict_proba", "predict", "score", "reliability", "ranking", "predict_topk", "error_analysis", "score_interval", "compare",
             "conformalize", "predict_set", "coverage")


@pytest.mark.parametrize("name", CONSUMERS)
def test_every_consumer_is_one_function_defined_in_the_mixin(name):
    from slnlp.ensemble import VotingEnsemble
    from slnlp.judge import LogProbJudge
    from slnlp.net import NeuralNetClassifier
    fn = getattr(NeuralNetClassifier, name)
    assert fn is getattr(VotingEnsemble, name) and fn is LogProbJudge.__dict__[name]
    assert fn.__module__ == "slnlp.judge"
    assert name not in NeuralNetClassifier.__dict__ and name not in VotingEnsemble.__dict__


def test_a_consumer_added_to_the_mixin_exists_on_both_estimators():
    from slnlp.ensemble import VotingEnsemble
    from slnlp.judge import LogProbJudge
    from slnlp.net import NeuralNetClassifier

    class Judge(LogProbJudge):                               # a throwaway mixin with one more consumer; the product is not touched
        def top_class_margin(self, X):
            return self._judge(self._as_dataset(X), lambda logp, yd: logp)

    for base in (NeuralNetClassifier, VotingEnsemble):
        assert issubclass(base, LogProbJudge) and not hasattr(base, "top_class_margin")
        sub = type("Sub", (Judge, base), {})
        assert sub.top_class_margin is Judge.top_class_margin
        assert sub.ranking is LogProbJudge.ranking and sub._forward_logp is base._forward_logp
