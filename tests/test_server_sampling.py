"""POST /tts with the sampling fields (temperature, top_k, seed), on a fake service (CPU): they reach
``service.submit`` as a ``Sampling``, a body of only ``text`` calls ``submit(text)`` with that one
argument as before, and invalid values give 422."""
import numpy as np
import pytest

from llmvox_amd.sampling import Sampling


class _OldService:
    """The fake of tests/test_server.py: submit takes the text alone."""

    def __init__(self):
        self.error = None
        self.sessions = []
        self.texts = []

    def submit(self, text):
        self.texts.append(text)
        return text

    def chunks(self, session):
        yield np.zeros(320, dtype=np.float32).tobytes()


class _Service(_OldService):
    def __init__(self):
        super().__init__()
        self.calls = []

    def submit(self, *args, **kw):
        self.calls.append((args, kw))
        return args[0]


@pytest.fixture
def client_of():
    from fastapi.testclient import TestClient
    from llmvox_amd.server import create_app
    return lambda svc, **kw: TestClient(create_app(svc, **kw))


def test_fields_reach_submit_as_a_sampling(client_of):
    svc = _Service()
    client = client_of(svc)
    r = client.post("/tts", json={"text": "hello.", "temperature": 0.8, "top_k": 50, "seed": 1234567890123})
    assert r.status_code == 200 and len(r.content) == 1280
    assert svc.calls == [(("hello.",), {"sampling": Sampling(0.8, 50, 1234567890123)})]
    # no seed with a temperature > 0: one is drawn per request
    for _ in range(2):
        assert client.post("/tts", json={"text": "hello.", "temperature": 1.0}).status_code == 200
    a, b = (kw["sampling"] for _, kw in svc.calls[1:])
    assert (a.temperature, a.top_k) == (1.0, 0) and isinstance(a.seed, int) and 0 <= a.seed < 2 ** 64
    assert a.seed != b.seed
    # temperature 0 is greedy, whatever else is named
    svc.calls.clear()
    assert client.post("/tts", json={"text": "hello.", "temperature": 0, "top_k": 5, "seed": 3}).status_code == 200
    assert svc.calls == [(("hello.",), {})]


def test_text_only_body_calls_submit_with_one_argument(client_of):
    old = _OldService()
    assert client_of(old).post("/tts", json={"text": "hello world."}).status_code == 200
    assert old.texts == ["hello world."]
    svc = _Service()
    assert client_of(svc).post("/tts", json={"text": "hello world."}).status_code == 200
    assert svc.calls == [(("hello world.",), {})]


@pytest.mark.parametrize("body", ['{"text": "x", "temperature": -1}', '{"text": "x", "temperature": NaN}',
                                  '{"text": "x", "temperature": 1.0, "top_k": -1}',
                                  '{"text": "x", "temperature": Infinity}', '{"text": "x", "temperature": 1, "seed": -5}',
                                  '{"text": "x", "temperature": "warm"}', '{"text": "x", "top_k": -1}'],
                         ids=["temperature-neg", "temperature-nan", "top_k-neg", "temperature-inf", "seed-neg",
                              "temperature-str", "top_k-neg-alone"])
def test_invalid_values_give_422(client_of, body):
    svc = _Service()
    r = client_of(svc).post("/tts", content=body, headers={"content-type": "application/json"})
    assert r.status_code == 422, r.text
    assert svc.calls == []


def test_server_defaults_apply_to_requests_that_name_no_field(client_of):
    svc = _Service()
    client = client_of(svc, temperature=0.7, top_k=40)
    assert client.post("/tts", json={"text": "a."}).status_code == 200
    (args, kw), = svc.calls
    assert args == ("a.",) and (kw["sampling"].temperature, kw["sampling"].top_k) == (0.7, 40)
    svc.calls.clear()
    assert client.post("/tts", json={"text": "a.", "temperature": 0}).status_code == 200  # asks for greedy
    assert svc.calls == [(("a.",), {})]
    with pytest.raises(ValueError):
        client_of(svc, temperature=-1.0)
